// sigcache_sanitize_main.cpp -- TEST HARNESS ONLY.  An executable that runs the
// verified-ID cache's code (hostemu_sigcache.cpp over stl_sigcache_core.h)
// under AddressSanitizer + UndefinedBehaviorSanitizer, built and started by
// tests/test_sigcache_host.py.  Every array handed to the code is an exactly
// sized heap buffer, and the cache's lines are one too, so a read or write
// outside them is an ASan report.
//
//   argv[1]  written by the test: u64 seed, u32 n, n 32-byte IDs.
// For sets_log2 0, 2 and 10: the IDs go in in batches of 1, 2, 3, ... (every
// other row of every other batch held back by its accept byte), then every ID
// is looked up.  Checked here: an ID that was never inserted is absent, one
// whose set received at most four distinct IDs is present, a fuller set holds
// at most four, the all-zero ID and a half-written slot hit nothing, and a
// cleared cache is empty.
// Exit status = number of failed checks; any sanitizer report aborts.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "hostemu_sigcache.cpp"

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
  uint8_t* p = static_cast<uint8_t*>(std::malloc(bytes ? bytes : 1));
  if (bytes) std::memcpy(p, src, bytes);
  return p;
}

static void insert_exact(void* c, const uint8_t* ids, size_t m, const uint8_t* accept) {
  uint8_t* a = exact(ids, 32 * m);
  uint8_t* f = accept ? exact(accept, m) : nullptr;
  hostemu_sigcache_insert(c, a, m, f);
  std::free(a);
  std::free(f);
}

static std::vector<uint8_t> lookup_exact(void* c, const uint8_t* ids, size_t m) {
  uint8_t* a = exact(ids, 32 * m);
  uint8_t* h = static_cast<uint8_t*>(std::malloc(m ? m : 1));
  hostemu_sigcache_lookup(c, a, m, h);
  std::vector<uint8_t> out(h, h + m);
  std::free(a);
  std::free(h);
  return out;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string data = slurp(argv[1]);
  if (data.size() < 12) return 2;
  uint64_t seed;
  uint32_t n;
  std::memcpy(&seed, data.data(), 8);
  std::memcpy(&n, data.data() + 8, 4);
  if (data.size() != 12 + 32 * (size_t)n) return 2;
  const uint8_t* ids = reinterpret_cast<const uint8_t*>(data.data()) + 12;
  const uint8_t zero[32] = {0};
  for (uint32_t k : {0u, 2u, 10u}) {
    void* c = hostemu_sigcache_create(k, seed);
    CHECK(c != nullptr, "create %u", k);
    if (!c) continue;
    std::map<uint32_t, std::set<std::string>> sets;
    std::set<std::string> inserted;
    size_t at = 0, batch = 1;
    while (at < n) {
      const size_t m = std::min<size_t>(batch, n - at);
      std::vector<uint8_t> accept(m, 1);
      const bool held = batch % 2 == 0;
      for (size_t i = 0; i < m; ++i) {
        if (held && i % 2 == 1) accept[i] = 0;
        if (!accept[i]) continue;
        const std::string id(reinterpret_cast<const char*>(ids + 32 * (at + i)), 32);
        inserted.insert(id);
        sets[hostemu_sigcache_set(hostemu_sigcache_hash(ids + 32 * (at + i), seed), k)].insert(id);
      }
      insert_exact(c, ids + 32 * at, m, held ? accept.data() : nullptr);
      at += m;
      ++batch;
    }
    const std::vector<uint8_t> hit = lookup_exact(c, ids, n);
    std::map<uint32_t, int> present;
    for (uint32_t i = 0; i < n; ++i) {
      const std::string id(reinterpret_cast<const char*>(ids + 32 * i), 32);
      const uint32_t s = hostemu_sigcache_set(hostemu_sigcache_hash(ids + 32 * i, seed), k);
      if (!inserted.count(id)) CHECK(!hit[i], "log2 %u: row %u was never inserted", k, i);
      else if (sets[s].size() <= 4) CHECK(hit[i], "log2 %u: row %u of a set of %zu is absent", k, i, sets[s].size());
    }
    for (const auto& kv : sets) {
      int there = 0;
      for (const std::string& id : kv.second)
        there += lookup_exact(c, reinterpret_cast<const uint8_t*>(id.data()), 1)[0];
      CHECK(there <= 4 && there >= (int)std::min<size_t>(4, kv.second.size()), "log2 %u: set %u holds %d of %zu", k,
            kv.first, there, kv.second.size());
    }
    CHECK(!lookup_exact(c, zero, 1)[0], "log2 %u: the zero ID hits", k);
    insert_exact(c, zero, 1, nullptr);
    CHECK(!lookup_exact(c, zero, 1)[0], "log2 %u: the zero ID was stored", k);
    hostemu_sigcache_clear(c);
    const std::vector<uint8_t> after = lookup_exact(c, ids, n);
    for (uint32_t i = 0; i < n; ++i) CHECK(!after[i], "log2 %u: row %u survives a clear", k, i);
    // a half-written slot: the first 8 bytes of an ID in every way of its set, zeros behind
    if (n > 0) {
      uint32_t* lines = hostemu_sigcache_lines(c);
      const uint32_t s = hostemu_sigcache_set(hostemu_sigcache_hash(ids, seed), k);
      for (int w = 0; w < 4; ++w) std::memcpy(lines + 32 * (size_t)s + 8 * w, ids, 8);
      CHECK(!lookup_exact(c, ids, 1)[0], "log2 %u: a half-written slot hits", k);
    }
    hostemu_sigcache_destroy(c);
    std::printf("log2 %u: sets %zu inserted %zu\n", k, sets.size(), inserted.size());
  }
  std::printf("ids %u\nfailed checks %ld\n", n, g_bad);
  return g_bad > 255 ? 255 : (int)g_bad;
}
