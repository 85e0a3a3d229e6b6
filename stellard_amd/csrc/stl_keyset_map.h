// stl_keyset_map.h -- the key -> index map of a registered signer set
// (stl_keyset_*): what stl_keyset_find answers on the host, in a form a
// kernel can probe.
//
// Open addressing with linear probing over a power-of-two number of slots,
// at least 4 per key (a load of 1/4 at most).  A slot is the key's index in
// the set, or kKsMapEmpty; the key bytes are not stored again: a probe
// compares the row's 32 bytes with the first 8 words of the key's record
// (stl_comb.h: words 0-7 of a record are the encoding as registered).  Of a
// key registered more than once only the first index is in the map.
//
// The hash takes a 64-bit seed.  The builder tries the seeds 0, 1, 2, ... and
// keeps the first under which no key lies further than kKsMapProbeBound slots
// from its home slot; the longest distance it measured is kept with the map
// and is as far as a lookup ever probes.  So the registered keys cannot be
// chosen to make lookups slow (a set that is bad for one seed gets the next),
// and a key that is not registered costs at most that many slots.
//
// Plain C++: the hash and the probe compile for the host and the device, the
// builder for the host only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace stl {

constexpr uint32_t kKsMapEmpty = 0xFFFFFFFFu;  // an empty slot; a lookup's "not found"
constexpr uint32_t kKsMapSlotsPerKey = 4;
// Longest probe sequence a built map may have.  At a load of 1/4 the longest
// run of 4,096 random keys is about 13 slots, so seed 0 serves any set that
// was not made to collide.
constexpr uint32_t kKsMapProbeBound = 32;
constexpr uint32_t kKsMapMaxSeeds = 256;  // the build fails after this many

#define STL_MAP_HD __host__ __device__ inline

// Slots of the map of nkeys keys: the power of two >= 4 * nkeys (4 at least).
STL_MAP_HD uint32_t keyset_map_slots(uint32_t nkeys) {
  uint32_t s = 4;
  while (s < kKsMapSlotsPerKey * nkeys) s <<= 1;
  return s;
}

STL_MAP_HD uint64_t keyset_map_mix(uint64_t h) {
  h ^= h >> 32;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 29;
  return h;
}

// 32-bit hash of the eight key words under `seed` (every word and the whole
// seed reach every bit of the result).
STL_MAP_HD uint32_t keyset_map_hash(const uint32_t k[8], uint64_t seed) {
  uint64_t h = keyset_map_mix(seed + 0x9e3779b97f4a7c15ull);
#pragma unroll
  for (int i = 0; i < 4; ++i) h = keyset_map_mix((h ^ (k[2 * i] | ((uint64_t)k[2 * i + 1] << 32))) * 0xc4ceb9fe1a85ec53ull);
  h = keyset_map_mix(h + seed * 0xd6e8feb86659fd93ull);
  return (uint32_t)(h >> 32);
}

// The index of key k, or kKsMapEmpty.  slots: mask + 1 of them; keys: the
// registered keys' bytes as words, key i at keys + i * stride (the records on
// the device, stride kKeyRecWords; the plain key array on the host, stride
// 8); max_probe: the map's longest probe sequence.
STL_MAP_HD uint32_t keyset_map_probe(const uint32_t* slots, uint32_t mask, uint64_t seed, uint32_t max_probe,
                                     const uint32_t* keys, uint32_t stride, const uint32_t k[8]) {
  uint32_t at = keyset_map_hash(k, seed) & mask;
  for (uint32_t i = 0; i < max_probe; ++i, at = (at + 1) & mask) {
    const uint32_t idx = slots[at];
    if (idx == kKsMapEmpty) return kKsMapEmpty;
    const uint32_t* r = keys + (size_t)idx * stride;
    uint32_t diff = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) diff |= r[w] ^ k[w];
    if (diff == 0) return idx;
  }
  return kKsMapEmpty;
}

// A built map: slots.size() is a power of two, `longest` <= kKsMapProbeBound.
struct KeysetMap {
  std::vector<uint32_t> slots;
  uint64_t seed = 0;
  uint32_t longest = 0;
  uint32_t mask() const { return (uint32_t)slots.size() - 1; }
};

// Builds the map of the keys pk32[0 .. nkeys) (8 words each, 4-byte aligned);
// first[0 .. nfirst): the index of each distinct key's first appearance, in
// the order they are inserted.  false: no seed below kKsMapMaxSeeds keeps
// the longest probe sequence within the bound.
inline bool keyset_map_build(KeysetMap& m, const uint32_t* pk32, uint32_t nkeys, const uint32_t* first,
                             uint32_t nfirst) {
  const uint32_t nslots = keyset_map_slots(nkeys), mask = nslots - 1;
  for (uint64_t seed = 0; seed < kKsMapMaxSeeds; ++seed) {
    m.slots.assign(nslots, kKsMapEmpty);
    uint32_t longest = 0;
    for (uint32_t j = 0; j < nfirst && longest <= kKsMapProbeBound; ++j) {
      uint32_t at = keyset_map_hash(pk32 + 8 * (size_t)first[j], seed) & mask, len = 1;
      while (m.slots[at] != kKsMapEmpty && len <= kKsMapProbeBound) {
        at = (at + 1) & mask;
        ++len;
      }
      if (len <= kKsMapProbeBound) m.slots[at] = first[j];
      longest = len > longest ? len : longest;
    }
    if (longest <= kKsMapProbeBound) {
      m.seed = seed;
      m.longest = longest;
      return true;
    }
  }
  m.slots.clear();
  return false;
}

}  // namespace stl
