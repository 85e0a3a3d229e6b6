// shamap_tree_sanitize_main.cpp -- TEST HARNESS ONLY.  An executable that runs
// the resident SHAMap's code (hostemu_shamap_tree.cpp over
// stl_shamap_tree_core.h) under AddressSanitizer + UndefinedBehaviorSanitizer,
// built and started by tests/test_shamap_tree_host.py.  Every array handed to
// the code is an exactly sized heap buffer, and the emulation's own arrays (the
// generations, the compacted changes, the scratch) are exactly sized vectors,
// so a read or write outside one is an ASan report.
//
//   argv[1]  written by the test: u32 sequences, then per sequence u32
//            capacity, u32 steps, and per step u32 n, u8 leaf hashes given, u8
//            ops given, n keys, (n leaf hashes,) (n op bytes,) i32 the expected
//            return code, the model's root, its 8 counts, u32 items and the
//            items' sorted keys and leaf hashes.
// Checked here: the return code; root, counts and exported content equal the
// model's (after a refused step: unchanged).
// Exit status = number of failed checks; any sanitizer report aborts.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "hostemu_shamap_tree.cpp"

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
  const uint32_t seqs = u32();
  uint32_t steps_run = 0;
  for (uint32_t si = 0; si < seqs; ++si) {
    const uint32_t cap = u32(), steps = u32();
    void* tree = hostemu_tree_new(cap);
    for (uint32_t st = 0; st < steps; ++st, ++steps_run) {
      const uint32_t n = u32();
      const bool has_leaf = *at++ != 0, has_op = *at++ != 0;
      uint8_t* key = exact(at, 32 * (size_t)n);
      at += 32 * (size_t)n;
      uint8_t* leaf = has_leaf ? exact(at, 32 * (size_t)n) : nullptr;
      if (has_leaf) at += 32 * (size_t)n;
      uint8_t* op = has_op ? exact(at, n) : nullptr;
      if (has_op) at += n;
      const int32_t want_rc = (int32_t)u32();
      const uint8_t* want_root = at;
      at += 32;
      uint32_t want[8];
      std::memcpy(want, at, 32);
      at += 32;
      const uint32_t items = u32();
      const uint8_t* want_keys = at;
      at += 32 * (size_t)items;
      const uint8_t* want_leaves = at;
      at += 32 * (size_t)items;
      if (at > end) return 98;
      uint8_t* root = static_cast<uint8_t*>(std::malloc(32));
      uint32_t* cnt = static_cast<uint32_t*>(std::calloc(8, 4));
      const int rc = hostemu_tree_apply(tree, key, leaf, op, n, root, cnt);
      CHECK(rc == want_rc, "sequence %u step %u: rc %d want %d", si, st, rc, want_rc);
      if (rc == 0) {
        CHECK(std::memcmp(root, want_root, 32) == 0, "sequence %u step %u: root differs", si, st);
        CHECK(std::memcmp(cnt, want, 32) == 0, "sequence %u step %u: counts %u %u %u %u %u %u %u %u", si, st, cnt[0],
              cnt[1], cnt[2], cnt[3], cnt[4], cnt[5], cnt[6], cnt[7]);
      }
      uint8_t* ek = static_cast<uint8_t*>(std::malloc(32 * (size_t)cap));
      uint8_t* el = static_cast<uint8_t*>(std::malloc(32 * (size_t)cap));
      const uint32_t m = hostemu_tree_export(tree, ek, el);
      CHECK(m == items, "sequence %u step %u: %u items want %u", si, st, m, items);
      if (m == items) {
        CHECK(std::memcmp(ek, want_keys, 32 * (size_t)m) == 0, "sequence %u step %u: keys differ", si, st);
        CHECK(std::memcmp(el, want_leaves, 32 * (size_t)m) == 0, "sequence %u step %u: leaf hashes differ", si, st);
      }
      std::printf("sequence %u step %u: n %u rc %d items %u dirty %u gathered %u\n", si, st, n, rc, m, cnt[6], cnt[7]);
      std::free(key);
      std::free(leaf);
      std::free(op);
      std::free(root);
      std::free(cnt);
      std::free(ek);
      std::free(el);
    }
    hostemu_tree_free(tree);
  }
  std::printf("steps %u failed checks %ld\n", steps_run, g_bad);
  return g_bad > 250 ? 250 : (int)g_bad;
}
