// shamap_nodes_sanitize_main.cpp -- TEST HARNESS ONLY.  An executable that runs
// the node-storing computations (hostemu_shamap_nodes.cpp over
// stl_shamap_core.h and stl_shamap_tree_core.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer, built and started by
// tests/test_shamap_nodes_host.py.  Every array handed to the code is an
// exactly sized heap buffer -- the four output arrays hold max_nodes rows and
// not one more -- so a read or write outside one is an ASan report.
//
//   argv[1]  written by the test: u32 cases, then per case
//            u8 kind (0: a set, 1: an apply), u32 max_nodes;
//            an apply only: u32 m_old, m_old keys, m_old leaf hashes;
//            u32 n, u8 leaf hashes given, u8 select / ops given, n keys,
//            (n leaf hashes,) (ceil(n / 8) select bytes | n op bytes,)
//            the model's root and its node count.
// Checked here: root and count equal the model's; every row written hashes
// ("MIN\0" || body) to its hash, its depth is in 0 .. 63, bits 8-15 of its meta
// word are clear and its ID is its own masked self.
// Exit status = number of failed checks; any sanitizer report aborts.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "hostemu_shamap_nodes.cpp"

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
  auto take = [&](size_t bytes) {
    uint8_t* p = exact(at, bytes);
    at += bytes;
    return p;
  };
  const uint32_t cases = u32();
  unsigned long long stored = 0;
  for (uint32_t ci = 0; ci < cases; ++ci) {
    const bool apply = *at++ != 0;
    const uint32_t max_nodes = u32();
    uint32_t m_old = 0;
    uint8_t *old_key = nullptr, *old_leaf = nullptr;
    if (apply) {
      m_old = u32();
      old_key = take(32 * (size_t)m_old);
      old_leaf = take(32 * (size_t)m_old);
    }
    const uint32_t n = u32();
    const bool has_leaf = *at++ != 0, has_extra = *at++ != 0;
    uint8_t* key = take(32 * (size_t)n);
    uint8_t* leaf = has_leaf ? take(32 * (size_t)n) : nullptr;
    uint8_t* extra = has_extra ? take(apply ? n : (n + 7) / 8) : nullptr;
    const uint8_t* want_root = at;
    at += 32;
    const uint32_t want_count = u32();
    if (at > end) return 98;
    uint8_t* root = static_cast<uint8_t*>(std::malloc(32));
    uint8_t* hash = static_cast<uint8_t*>(std::malloc(32 * (size_t)max_nodes + 1));
    uint8_t* body = static_cast<uint8_t*>(std::malloc(512 * (size_t)max_nodes + 1));
    uint8_t* id = static_cast<uint8_t*>(std::malloc(32 * (size_t)max_nodes + 1));
    uint32_t* meta = static_cast<uint32_t*>(std::malloc(4 * (size_t)max_nodes + 4));
    uint32_t* count = static_cast<uint32_t*>(std::malloc(4));
    // the one spare byte (word) keeps malloc(0) out of it; it is a guard
    hash[32 * (size_t)max_nodes] = body[512 * (size_t)max_nodes] = id[32 * (size_t)max_nodes] = 0xA5;
    meta[max_nodes] = 0xA5A5A5A5u;
    int rc;
    if (apply) {
      uint8_t* nk = static_cast<uint8_t*>(std::malloc(32 * (size_t)(m_old + n)));
      uint8_t* nl = static_cast<uint8_t*>(std::malloc(32 * (size_t)(m_old + n)));
      uint32_t info[3];
      rc = hostemu_nodes_apply(old_key, old_leaf, m_old, key, leaf, extra, n, nk, nl, root, info, max_nodes, hash,
                               body, id, meta, count);
      std::free(nk);
      std::free(nl);
    } else {
      uint32_t* cnt = static_cast<uint32_t*>(std::malloc(16));
      rc = hostemu_nodes_set(key, leaf, extra, n, root, cnt, max_nodes, hash, body, id, meta, count);
      CHECK(rc != 0 || cnt[2] == *count, "case %u: counts[2] %u, count %u", ci, cnt[2], *count);
      std::free(cnt);
    }
    CHECK(rc == 0, "case %u: rc %d", ci, rc);
    if (rc == 0) {
      CHECK(std::memcmp(root, want_root, 32) == 0, "case %u: root differs", ci);
      CHECK(*count == want_count, "case %u: count %u want %u", ci, *count, want_count);
      const uint32_t rows = *count < max_nodes ? *count : max_nodes;
      for (uint32_t r = 0; r < rows; ++r) {
        uint32_t rec[stl::kShamapRecordWords], h[8], idw[8], again[8];
        rec[0] = stl::kShamapInnerPrefix;
        std::memcpy(rec + 1, body + 512 * (size_t)r, 512);
        stl::shamap_inner_hash(h, rec);
        CHECK(std::memcmp(h, hash + 32 * (size_t)r, 32) == 0, "case %u row %u: the body does not hash to the hash", ci, r);
        const uint32_t d = meta[r] & 0xffu;
        CHECK(d < 64 && (meta[r] & 0xff00u) == 0, "case %u row %u: meta %08x", ci, r, meta[r]);
        std::memcpy(idw, id + 32 * (size_t)r, 32);
        stl::shamap_mask_key(again, idw, d);
        CHECK(std::memcmp(again, idw, 32) == 0, "case %u row %u: the ID has nibbles past its depth", ci, r);
      }
      stored += rows;
      CHECK(hash[32 * (size_t)max_nodes] == 0xA5 && body[512 * (size_t)max_nodes] == 0xA5 &&
                id[32 * (size_t)max_nodes] == 0xA5 && meta[max_nodes] == 0xA5A5A5A5u,
            "case %u: a guard behind row max_nodes was written", ci);
      std::printf("case %u: %s n %u max_nodes %u count %u\n", ci, apply ? "apply" : "set", n, max_nodes, *count);
    }
    std::free(old_key);
    std::free(old_leaf);
    std::free(key);
    std::free(leaf);
    std::free(extra);
    std::free(root);
    std::free(hash);
    std::free(body);
    std::free(id);
    std::free(meta);
    std::free(count);
  }
  std::printf("cases %u rows %llu failed checks %ld\n", cases, stored, g_bad);
  return g_bad > 250 ? 250 : (int)g_bad;
}
