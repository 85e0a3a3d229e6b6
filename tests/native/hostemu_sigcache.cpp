// hostemu_sigcache.cpp -- TEST HARNESS ONLY.  Compiles the verified-ID cache's
// device code (stellard_amd/csrc/stl_sigcache_core.h) for the host: the hash,
// the probe and the insert as they are (the compare-and-swap of one thread),
// and a lookup over arrays as sigcache_lookup_kernel runs it, row by row.  Not
// part of the product library.
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../stellard_amd/csrc/stl_sigcache_core.h"

namespace {

struct EmuCache {
  uint32_t sets_log2 = 0, mask = 0;
  uint64_t seed = 0;
  uint32_t* lines = nullptr;  // exactly 32 * (mask + 1) words, 128-byte aligned
};

void load_id(uint32_t w[stl::kScIdWords], const uint8_t* id) { std::memcpy(w, id, 32); }

}  // namespace

extern "C" {

uint64_t hostemu_sigcache_hash(const uint8_t id[32], uint64_t seed) {
  uint32_t w[stl::kScIdWords];
  load_id(w, id);
  return stl::sigcache_hash(w, seed);
}

uint32_t hostemu_sigcache_set(uint64_t hash, uint32_t sets_log2) {
  return stl::sigcache_set(hash, (1u << sets_log2) - 1u);
}

uint32_t hostemu_sigcache_first_way(uint64_t hash) { return stl::sigcache_first_way(hash); }

uint64_t hostemu_sigcache_bytes(uint32_t sets_log2) { return stl::sigcache_bytes(sets_log2); }

uint32_t hostemu_sigcache_predicate(uint32_t flags) { return stl::sigcache_predicate(flags); }

void* hostemu_sigcache_create(uint32_t sets_log2, uint64_t seed) {
  if (sets_log2 > stl::kScLog2Max) return nullptr;
  EmuCache* c = new EmuCache();
  c->sets_log2 = sets_log2;
  c->mask = (1u << sets_log2) - 1u;
  c->seed = seed;
  void* p = nullptr;
  if (posix_memalign(&p, 128, stl::sigcache_bytes(sets_log2)) != 0) {
    delete c;
    return nullptr;
  }
  c->lines = static_cast<uint32_t*>(p);
  std::memset(c->lines, 0, stl::sigcache_bytes(sets_log2));
  return c;
}

void hostemu_sigcache_destroy(void* h) {
  EmuCache* c = static_cast<EmuCache*>(h);
  if (!c) return;
  std::free(c->lines);
  delete c;
}

void hostemu_sigcache_clear(void* h) {
  EmuCache* c = static_cast<EmuCache*>(h);
  std::memset(c->lines, 0, stl::sigcache_bytes(c->sets_log2));
}

// sigcache_insert_kernel, row by row: accept (nullable) holds one byte per
// row, rows with 0 are not inserted.
void hostemu_sigcache_insert(void* h, const uint8_t* ids, size_t n, const uint8_t* accept) {
  EmuCache* c = static_cast<EmuCache*>(h);
  for (size_t i = 0; i < n; ++i) {
    if (accept && !accept[i]) continue;
    uint32_t w[stl::kScIdWords];
    load_id(w, ids + 32 * i);
    stl::sigcache_insert(c->lines, c->mask, c->seed, w, stl::ScCasHost{});
  }
}

// sigcache_lookup_kernel, row by row: hit[i] = 1 / 0.
void hostemu_sigcache_lookup(void* h, const uint8_t* ids, size_t n, uint8_t* hit) {
  const EmuCache* c = static_cast<const EmuCache*>(h);
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[stl::kScIdWords];
    load_id(w, ids + 32 * i);
    hit[i] = stl::sigcache_probe(c->lines, c->mask, c->seed, w) ? 1 : 0;
  }
}

// The lines themselves (32 * 2^sets_log2 words), for tests that write a slot
// by hand.
uint32_t* hostemu_sigcache_lines(void* h) { return static_cast<EmuCache*>(h)->lines; }

}  // extern "C"
