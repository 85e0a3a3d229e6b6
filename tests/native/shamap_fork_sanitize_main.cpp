// shamap_fork_sanitize_main.cpp -- TEST HARNESS ONLY.  An executable that runs
// the resident SHAMap's fork, snapshot and revert (hostemu_shamap_fork.cpp over
// stl_shamap_tree_core.h) under AddressSanitizer + UndefinedBehaviorSanitizer,
// built and started by tests/test_shamap_fork_host.py.  The two trees'
// generations are vectors of exactly their own capacity and every array handed
// to the code is an exactly sized heap buffer, so a read of the source past its
// capacity or a store into the destination past its own is an ASan report --
// with the source larger than the destination and the reverse.
//
//   argv[1]  written by the test: u32 cases, then per case u32 source capacity,
//            u32 destination capacity, u32 items loaded into the source with
//            their keys and leaf hashes, u32 the source's stated count
//            afterwards (0xffffffff: as it is), u32 items loaded into the
//            destination with keys and leaf hashes, the fork's batch (u32 n, u8
//            leaf hashes given, u8 ops given, n keys, (n leaf hashes,) (n op
//            bytes,)), i32 the expected return code, the model's root and 8
//            counts, u32 items and the destination's sorted keys and leaf
//            hashes afterwards (after a refusal: what it held).
// Checked here: the return code, root, counts, the destination's content, the
// source byte-equal before and after, and the destination's revert: allowed
// after a fork that succeeded (and gives back what it held), refused otherwise.
// Exit status = number of failed checks; any sanitizer report aborts.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "hostemu_shamap_fork.cpp"

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

struct Content {
  uint32_t items = 0;
  std::vector<uint8_t> key, leaf, root;
  Content(void* tree, uint32_t cap) : key(32 * (size_t)cap), leaf(32 * (size_t)cap), root(32) {
    items = hostemu_fork_export(tree, key.data(), leaf.data(), root.data());
  }
  bool operator==(const Content& o) const { return items == o.items && key == o.key && leaf == o.leaf && root == o.root; }
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
  auto load = [&](void* tree, uint32_t items) {
    uint8_t* k = exact(at, 32 * (size_t)items);
    at += 32 * (size_t)items;
    uint8_t* l = exact(at, 32 * (size_t)items);
    at += 32 * (size_t)items;
    uint8_t root[32];
    const int rc = hostemu_fork_apply(tree, k, l, nullptr, items, root, nullptr);
    std::free(k);
    std::free(l);
    return rc;
  };
  const uint32_t cases = u32();
  for (uint32_t ci = 0; ci < cases; ++ci) {
    const uint32_t scap = u32(), dcap = u32();
    void* src = hostemu_fork_new(scap);
    void* dst = hostemu_fork_new(dcap);
    const uint32_t sitems = u32();
    CHECK(load(src, sitems) == 0, "case %u: the source's load", ci);
    const uint32_t stated = u32();
    if (stated != 0xffffffffu) hostemu_fork_state_count(src, stated);
    const uint32_t ditems = u32();
    CHECK(load(dst, ditems) == 0, "case %u: the destination's load", ci);
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
    const Content src_before(src, scap), dst_before(dst, dcap);
    uint8_t* root = static_cast<uint8_t*>(std::malloc(32));
    uint32_t* cnt = static_cast<uint32_t*>(std::calloc(8, 4));
    const int rc = hostemu_fork_fork(src, dst, key, leaf, op, n, root, cnt);
    CHECK(rc == want_rc, "case %u: rc %d want %d", ci, rc, want_rc);
    const Content dst_after(dst, dcap);
    if (rc == 0) {
      CHECK(std::memcmp(root, want_root, 32) == 0, "case %u: root differs", ci);
      CHECK(std::memcmp(dst_after.root.data(), want_root, 32) == 0, "case %u: the destination's root differs", ci);
      CHECK(std::memcmp(cnt, want, 32) == 0, "case %u: counts %u %u %u %u %u %u %u %u", ci, cnt[0], cnt[1], cnt[2],
            cnt[3], cnt[4], cnt[5], cnt[6], cnt[7]);
    }
    CHECK(dst_after.items == items, "case %u: %u items want %u", ci, dst_after.items, items);
    if (dst_after.items == items) {
      CHECK(std::memcmp(dst_after.key.data(), want_keys, 32 * (size_t)items) == 0, "case %u: keys differ", ci);
      CHECK(std::memcmp(dst_after.leaf.data(), want_leaves, 32 * (size_t)items) == 0, "case %u: leaf hashes differ", ci);
    }
    CHECK(Content(src, scap) == src_before, "case %u: the source changed", ci);
    const int rv = hostemu_fork_revert(dst);
    CHECK(rv == (rc == 0 ? 0 : -3), "case %u: revert %d after rc %d", ci, rv, rc);
    CHECK(Content(dst, dcap) == dst_before, "case %u: the destination after the revert", ci);
    CHECK(hostemu_fork_revert(dst) == -3, "case %u: a second revert", ci);
    std::printf("case %u: source %u of %u into %u, n %u rc %d items %u\n", ci, sitems, scap, dcap, n, rc, dst_after.items);
    std::free(key);
    std::free(leaf);
    std::free(op);
    std::free(root);
    std::free(cnt);
    hostemu_fork_free(src);
    hostemu_fork_free(dst);
  }
  std::printf("cases %u failed checks %ld\n", cases, g_bad);
  return g_bad > 250 ? 250 : (int)g_bad;
}
