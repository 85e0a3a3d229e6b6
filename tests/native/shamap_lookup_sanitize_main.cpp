// shamap_lookup_sanitize_main.cpp -- TEST HARNESS ONLY.  An executable that runs
// the code of the resident SHAMap's read-only calls
// (hostemu_shamap_lookup.cpp over stl_shamap_lookup_core.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer, built and started by
// tests/test_shamap_lookup_host.py.  Every array handed to the code is an
// exactly sized heap buffer -- the generations' rows, the queries, the outputs
// of ceil(n / 64) words, n rows and max_rows rows -- and the emulation's own
// arrays are exactly sized vectors, so a read or write outside one is an ASan
// report.
//
//   argv[1]  written by the test: u32 cases, then per case the two generations
//            (u32 items, the sorted keys, the leaf hashes, 65,536 bucket counts,
//            65,536 bucket hashes), u32 queries with their keys and the model's
//            answers against generation a (u8 found, leaf hash, u32 position),
//            u32 max_rows, the model's 8 counts and min(counts[0], max_rows)
//            rows (key, u8 kind, leaf a, leaf b).
// Exit status = number of failed checks; any sanitizer report aborts.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "hostemu_shamap_lookup.cpp"

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

template <typename T>
static T* exact(const uint8_t* src, size_t bytes) {
  if (!bytes) return nullptr;
  T* p = static_cast<T*>(std::malloc(bytes));
  std::memcpy(p, src, bytes);
  return p;
}

struct GenBuf {
  uint32_t m = 0;
  uint8_t *key = nullptr, *leaf = nullptr, *bh = nullptr;
  uint32_t* bcnt = nullptr;
  const uint8_t* read(const uint8_t* at) {
    std::memcpy(&m, at, 4);
    at += 4;
    key = exact<uint8_t>(at, 32 * (size_t)m);
    at += 32 * (size_t)m;
    leaf = exact<uint8_t>(at, 32 * (size_t)m);
    at += 32 * (size_t)m;
    bcnt = exact<uint32_t>(at, 4 * (size_t)stl::kTreeBuckets);
    at += 4 * (size_t)stl::kTreeBuckets;
    bh = exact<uint8_t>(at, 32 * (size_t)stl::kTreeBuckets);
    return at + 32 * (size_t)stl::kTreeBuckets;
  }
  void release() {
    std::free(key);
    std::free(leaf);
    std::free(bcnt);
    std::free(bh);
  }
};

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
    GenBuf a, b;
    at = a.read(at);
    at = b.read(at);
    // the lookup
    const uint32_t n = u32();
    uint8_t* q = exact<uint8_t>(at, 32 * (size_t)n);
    at += 32 * (size_t)n;
    const uint8_t* want = at;  // n records of 1 + 32 + 4 bytes
    at += 37 * (size_t)n;
    if (at > end) return 98;
    const size_t nw = ((size_t)n + 63) / 64;
    uint64_t* words = static_cast<uint64_t*>(std::malloc(nw ? 8 * nw : 1));
    uint8_t* leaf = static_cast<uint8_t*>(std::malloc(n ? 32 * (size_t)n : 1));
    uint32_t* pos = static_cast<uint32_t*>(std::malloc(n ? 4 * (size_t)n : 1));
    hostemu_lookup(a.key, a.leaf, a.bcnt, a.m, q, n, words, leaf, pos);
    for (uint32_t i = 0; i < n; ++i) {
      const uint8_t* w = want + 37 * (size_t)i;
      uint32_t wp;
      std::memcpy(&wp, w + 33, 4);
      CHECK(((words[i >> 6] >> (i & 63)) & 1u) == w[0], "case %u query %u: found bit", ci, i);
      CHECK(std::memcmp(leaf + 32 * (size_t)i, w + 1, 32) == 0, "case %u query %u: leaf hash", ci, i);
      CHECK(pos[i] == wp, "case %u query %u: position %u want %u", ci, i, pos[i], wp);
    }
    if (n & 63u) CHECK((words[nw - 1] >> (n & 63u)) == 0, "case %u: tail bits set", ci);
    hostemu_lookup(a.key, a.leaf, a.bcnt, a.m, q, n, words, nullptr, nullptr);  // the nullable outputs
    // the compare, both ways round (the second unchecked but for the counts' symmetry)
    const uint32_t max_rows = u32();
    uint32_t wc[8];
    std::memcpy(wc, at, 32);
    at += 32;
    const uint32_t rows = wc[0] < max_rows ? wc[0] : max_rows;
    const uint8_t* wrows = at;  // records of 32 + 1 + 32 + 32 bytes
    at += 97 * (size_t)rows;
    if (at > end) return 98;
    uint8_t* key = static_cast<uint8_t*>(std::malloc(max_rows ? 32 * (size_t)max_rows : 1));
    uint8_t* kind = static_cast<uint8_t*>(std::malloc(max_rows ? max_rows : 1));
    uint8_t* la = static_cast<uint8_t*>(std::malloc(max_rows ? 32 * (size_t)max_rows : 1));
    uint8_t* lb = static_cast<uint8_t*>(std::malloc(max_rows ? 32 * (size_t)max_rows : 1));
    uint32_t* counts = static_cast<uint32_t*>(std::calloc(8, 4));
    int rc = hostemu_compare(a.key, a.leaf, a.bcnt, a.bh, a.m, b.key, b.leaf, b.bcnt, b.bh, b.m, max_rows, key, kind,
                             la, lb, counts);
    CHECK(rc == 0, "case %u: compare rc %d", ci, rc);
    CHECK(std::memcmp(counts, wc, 32) == 0, "case %u: counts %u %u %u %u %u %u %u %u", ci, counts[0], counts[1],
          counts[2], counts[3], counts[4], counts[5], counts[6], counts[7]);
    for (uint32_t i = 0; i < rows && rc == 0; ++i) {
      const uint8_t* w = wrows + 97 * (size_t)i;
      CHECK(std::memcmp(key + 32 * (size_t)i, w, 32) == 0 && kind[i] == w[32], "case %u row %u: key or kind", ci, i);
      CHECK(std::memcmp(la + 32 * (size_t)i, w + 33, 32) == 0 && std::memcmp(lb + 32 * (size_t)i, w + 65, 32) == 0,
            "case %u row %u: leaf hashes", ci, i);
    }
    uint32_t back[8] = {};
    rc = hostemu_compare(b.key, b.leaf, b.bcnt, b.bh, b.m, a.key, a.leaf, a.bcnt, a.bh, a.m, max_rows, key, kind,
                         nullptr, nullptr, back);
    CHECK(rc == 0 && back[0] == wc[0] && back[1] == wc[2] && back[2] == wc[1] && back[3] == wc[3] &&
              back[4] == wc[4] && back[5] == wc[5],
          "case %u: the compare the other way round", ci);
    std::printf("case %u: items %u %u queries %u differences %u rows %u buckets %u examined %u\n", ci, a.m, b.m, n,
                counts[0], rows, counts[4], counts[5]);
    for (void* p : {(void*)q, (void*)words, (void*)leaf, (void*)pos, (void*)key, (void*)kind, (void*)la, (void*)lb,
                    (void*)counts})
      std::free(p);
    a.release();
    b.release();
  }
  std::printf("cases %u failed checks %ld\n", cases, g_bad);
  return g_bad > 250 ? 250 : (int)g_bad;
}
