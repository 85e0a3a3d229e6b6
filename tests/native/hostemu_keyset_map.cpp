// hostemu_keyset_map.cpp -- TEST HARNESS ONLY.  The keyset's key -> index map
// (stellard_amd/csrc/stl_keyset_map.h: the builder stl_keyset_create runs and
// the hash and probe keyset_lookup_kernel runs) compiled for the host, for the
// CPU test suite.  A map is built over the plain key array, which then stands
// in for the device's records (stride 8 words instead of kKeyRecWords).
#include <cstdint>
#include <cstring>
#include <map>
#include <array>
#include <vector>

#include "../../stellard_amd/csrc/stl_keyset_map.h"

namespace {
struct EmuMap {
  std::vector<uint32_t> keys;  // nkeys * 8 words
  uint32_t nkeys = 0;
  stl::KeysetMap map;
};
}  // namespace

extern "C" {

uint32_t hostemu_keyset_map_bound(void) { return stl::kKsMapProbeBound; }
uint32_t hostemu_keyset_map_empty(void) { return stl::kKsMapEmpty; }

uint32_t hostemu_keyset_map_hash(const uint8_t* key32, uint64_t seed) {
  uint32_t k[8];
  std::memcpy(k, key32, 32);
  return stl::keyset_map_hash(k, seed);
}

// The map of pk[0 .. nkeys) as stl_keyset_create builds it: from the first
// index of every distinct key, in index order.  NULL when no seed serves.
void* hostemu_keyset_map_build(const uint8_t* pk, uint32_t nkeys) {
  EmuMap* m = new EmuMap();
  m->nkeys = nkeys;
  m->keys.resize((size_t)nkeys * 8);
  std::memcpy(m->keys.data(), pk, (size_t)nkeys * 32);
  std::map<std::array<uint8_t, 32>, uint32_t> first;
  std::vector<uint32_t> firsts;
  for (uint32_t i = 0; i < nkeys; ++i) {
    std::array<uint8_t, 32> a;
    std::memcpy(a.data(), pk + 32 * (size_t)i, 32);
    if (first.emplace(a, i).second) firsts.push_back(i);
  }
  if (!stl::keyset_map_build(m->map, m->keys.data(), nkeys, firsts.data(), (uint32_t)firsts.size())) {
    delete m;
    return nullptr;
  }
  return m;
}

void hostemu_keyset_map_free(void* h) { delete static_cast<EmuMap*>(h); }

// out[0] slots, out[1] longest probe sequence, out[2] / out[3] the seed's low / high word
void hostemu_keyset_map_info(const void* h, uint32_t out[4]) {
  const EmuMap* m = static_cast<const EmuMap*>(h);
  out[0] = (uint32_t)m->map.slots.size();
  out[1] = m->map.longest;
  out[2] = (uint32_t)m->map.seed;
  out[3] = (uint32_t)(m->map.seed >> 32);
}

// out[i] = the index of key[32 i ..], or the empty mark, probing as the kernel does.
void hostemu_keyset_map_probe(const void* h, const uint8_t* key, size_t n, uint32_t* out) {
  const EmuMap* m = static_cast<const EmuMap*>(h);
  for (size_t i = 0; i < n; ++i) {
    uint32_t k[8];
    std::memcpy(k, key + 32 * i, 32);
    out[i] = stl::keyset_map_probe(m->map.slots.data(), m->map.mask(), m->map.seed, m->map.longest, m->keys.data(), 8,
                                   k);
  }
}

}  // extern "C"
