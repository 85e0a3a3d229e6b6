// shamap_sanitize_main.cpp -- TEST HARNESS ONLY.  An executable that runs the
// SHAMap root's code (hostemu_shamap.cpp over stl_shamap_core.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer, built and started by
// tests/test_shamap_host.py.  Every array handed to the code is an exactly
// sized heap buffer, so a read or write outside one is an ASan report.
//
//   argv[1]  written by the test: u32 cases, then per case u32 n, u8 leaf
//            hashes given, u8 select given, n keys, (n leaf hashes,)
//            (ceil(n / 8) select bytes,) the model's root and its 4 counts.
// Checked here: root and counts equal the model's; the neighbour bytes stay
// in -1 .. 63 and the histogram sums to the node count.  The sorted keys and
// the hash slots the level step searches and reads are exactly sized heap
// arrays as well.
// Exit status = number of failed checks; any sanitizer report aborts.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "hostemu_shamap.cpp"

static long g_bad = 0;
#define CHECK(c, ...)             \
  do {                            \
    if (!(c)) {                   \
      if (g_bad < 20) {           \
        std::printf(__VA_ARGS__); \
        std::printf("\n");        \
      }                           \
      ++g_bad;                    \
    }                             \
  } while (0)

static std::string slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static uint8_t* exact(const uint8_t* src, size_t bytes) {
  if (!bytes) return nullptr;
  uint8_t* p = static_cast<uint8_t*>(std::malloc(bytes));
  std::memcpy(p, src, bytes);
  return p;
}

int main(int argc, char** argv) {
  if (argc < 2) return 99;
  const std::string data = slurp(argv[1]);
  const uint8_t* at = reinterpret_cast<const uint8_t*>(data.data());
  const uint8_t* end = at + data.size();
  auto u32 = [&]() {
    uint32_t v = 0;
    std::memcpy(&v, at, 4);
    at += 4;
    return v;
  };
  const uint32_t cases = u32();
  for (uint32_t ci = 0; ci < cases; ++ci) {
    const uint32_t n = u32();
    const bool has_leaf = *at++ != 0, has_sel = *at++ != 0;
    uint8_t* key = exact(at, 32 * (size_t)n);
    at += 32 * (size_t)n;
    uint8_t* leaf = has_leaf ? exact(at, 32 * (size_t)n) : nullptr;
    if (has_leaf) at += 32 * (size_t)n;
    uint8_t* sel = has_sel ? exact(at, (n + 7) / 8) : nullptr;
    if (has_sel) at += (n + 7) / 8;
    const uint8_t* want_root = at;
    at += 32;
    uint32_t want[4];
    std::memcpy(want, at, 16);
    at += 16;
    if (at > end) return 98;
    uint8_t* root = static_cast<uint8_t*>(std::malloc(32));
    uint32_t* cnt = static_cast<uint32_t*>(std::malloc(16));
    uint32_t* hist = static_cast<uint32_t*>(std::malloc(256));
    int8_t* l = static_cast<int8_t*>(std::malloc(n ? n : 1));
    const int rc = hostemu_shamap_root(key, leaf, sel, n, root, cnt, hist, l);
    CHECK(rc == 0, "case %u: rc %d", ci, rc);
    CHECK(std::memcmp(root, want_root, 32) == 0, "case %u: root differs", ci);
    CHECK(std::memcmp(cnt, want, 16) == 0, "case %u: counts %u %u %u %u want %u %u %u %u", ci, cnt[0], cnt[1], cnt[2],
          cnt[3], want[0], want[1], want[2], want[3]);
    uint32_t sum = 0;
    for (int d = 0; d < 64; ++d) sum += hist[d];
    CHECK(sum == cnt[2], "case %u: histogram sums to %u, nodes %u", ci, sum, cnt[2]);
    for (uint32_t j = 0; j < cnt[0]; ++j) CHECK(l[j] >= -1 && l[j] <= 63, "case %u: l[%u] = %d", ci, j, (int)l[j]);
    std::printf("case %u: n %u distinct %u duplicates %u nodes %u deepest %u\n", ci, n, cnt[0], cnt[1], cnt[2],
                cnt[3]);
    std::free(key);
    std::free(leaf);
    std::free(sel);
    std::free(root);
    std::free(cnt);
    std::free(hist);
    std::free(l);
  }
  std::printf("cases %u failed checks %ld\n", cases, g_bad);
  return g_bad > 250 ? 250 : (int)g_bad;
}
