// stl_sigcache.h -- launch interface between stl_api.cpp (host) and
// stl_sigcache.hip (gfx950 device code): the verified-ID cache (stl_sigcache_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace stl {

// A cache on the device: mask + 1 lines of 128 bytes (stl_sigcache_core.h),
// 128-byte aligned.
struct SigCacheDev {
  uint32_t* lines;
  uint32_t mask;
  uint64_t seed;
};

// One lane per row; ids (n * 32 bytes) 16-byte aligned.  A row whose status is
// STL_TX_OK probes the cache.  bitmap: ceil(n / 64) words, each written whole
// with its wave's hits (no memset; the last word's tail bits are zero).
// counts (zeroed by the caller): [0] += the misses (STL_TX_OK rows not hit),
// [1] += the hits; miss_rows (n words): the misses' row numbers, appended wave
// by wave in the order the waves reserve their places.  counters (nullable):
// [0] += the hits (stl_get_stats' accepted).
hipError_t launch_sigcache_probe(const SigCacheDev& c, const uint8_t* ids, const uint8_t* status, uint32_t n,
                                 uint64_t* bitmap, uint32_t* miss_rows, uint32_t* counts,
                                 unsigned long long* counters, hipStream_t stream);
// One lane per listed row j < m: where bit j of cwords is 1, the ID of row
// rows[j] (ids + 32 * rows[j]) is inserted.
hipError_t launch_sigcache_insert(const SigCacheDev& c, const uint32_t* rows, uint32_t m, const uint64_t* cwords,
                                  const uint8_t* ids, hipStream_t stream);
// The bare probe: bit i of hit_words = ids[32 i ..] is present; words as above.
hipError_t launch_sigcache_lookup(const SigCacheDev& c, const uint8_t* ids, uint32_t n, uint64_t* hit_words,
                                  hipStream_t stream);

}  // namespace stl
