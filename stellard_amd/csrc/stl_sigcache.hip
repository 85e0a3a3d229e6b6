// stl_sigcache.hip -- gfx950 kernels of the verified-ID cache (stl_sigcache_*).
// One lane per row, 256-lane workgroups, no LDS.
//
//   sigcache_probe_kernel   the rows of one verify call: hit bitmap, miss list,
//                           both counts
//   sigcache_insert_kernel  the accepted rows among the misses
//   sigcache_lookup_kernel  the bare probe of n IDs
//
// A probe reads its set's line with plain 16-byte loads and compares all 32
// bytes; what it may see of a concurrent insert is argued at the top of
// stl_sigcache_core.h.  An insert decides by what its compare-and-swaps
// return (device scope: they are performed at the memory side, past the L2 of
// the workgroup's XCD), never by a plain load of another workgroup's store.
#include "stl_sigcache.h"

#include "stl_sigcache_core.h"

namespace stl {

namespace {

constexpr uint32_t kScBlock = 256;  // 4 waves per workgroup

struct ScCasDevice {
  __device__ uint64_t operator()(uint32_t* p, uint64_t want) const {
    return atomicCAS(reinterpret_cast<unsigned long long*>(p), 0ull, (unsigned long long)want);
  }
};

__device__ __forceinline__ void sc_ld_id(uint32_t id[kScIdWords], const uint8_t* ids, size_t row) {
  const uint4* q = reinterpret_cast<const uint4*>(ids + 32 * row);
  const uint4 a = q[0], b = q[1];
  id[0] = a.x; id[1] = a.y; id[2] = a.z; id[3] = a.w;
  id[4] = b.x; id[5] = b.y; id[6] = b.z; id[7] = b.w;
}

__global__ __launch_bounds__(kScBlock) void sigcache_probe_kernel(
    const uint32_t* __restrict__ lines, uint32_t mask, uint64_t seed, const uint8_t* __restrict__ ids,
    const uint8_t* __restrict__ status, uint32_t n, uint64_t* __restrict__ bitmap, uint32_t* __restrict__ miss_rows,
    uint32_t* __restrict__ counts, unsigned long long* __restrict__ ctr) {
  const uint32_t lane = threadIdx.x & 63u;
  const size_t wbase = (size_t)blockIdx.x * kScBlock + (threadIdx.x & ~63u);
  if (wbase >= n) return;  // wave-uniform
  const size_t j = wbase + lane;
  bool hit = false, miss = false;
  if (j < n && status[j] == kScTxOk) {
    uint32_t id[kScIdWords];
    sc_ld_id(id, ids, j);
    hit = sigcache_probe(lines, mask, seed, id);
    miss = !hit;
  }
  const uint64_t hw = __ballot(hit);
  const uint64_t mw = __ballot(miss);
  if (lane == 0) {
    bitmap[wbase >> 6] = hw;
    if (hw != 0) {
      atomicAdd(&counts[1], (uint32_t)__popcll(hw));
      if (ctr) atomicAdd(&ctr[0], (unsigned long long)__popcll(hw));  // accepted (stl_get_stats)
    }
  }
  if (mw == 0) return;  // wave-uniform
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(&counts[0], (uint32_t)__popcll(mw));
  base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
  if (miss) miss_rows[base + (uint32_t)__popcll(mw & ((1ull << lane) - 1ull))] = (uint32_t)j;
}

__global__ __launch_bounds__(kScBlock) void sigcache_insert_kernel(uint32_t* lines, uint32_t mask, uint64_t seed,
                                                                   const uint32_t* __restrict__ rows, uint32_t m,
                                                                   const uint64_t* __restrict__ cwords,
                                                                   const uint8_t* __restrict__ ids) {
  const size_t j = (size_t)blockIdx.x * kScBlock + threadIdx.x;
  if (j >= m) return;
  if (!((cwords[j >> 6] >> (j & 63u)) & 1ull)) return;
  uint32_t id[kScIdWords];
  sc_ld_id(id, ids, rows[j]);
  sigcache_insert(lines, mask, seed, id, ScCasDevice{});
}

__global__ __launch_bounds__(kScBlock) void sigcache_lookup_kernel(const uint32_t* __restrict__ lines, uint32_t mask,
                                                                   uint64_t seed, const uint8_t* __restrict__ ids,
                                                                   uint32_t n, uint64_t* __restrict__ hit_words) {
  const uint32_t lane = threadIdx.x & 63u;
  const size_t wbase = (size_t)blockIdx.x * kScBlock + (threadIdx.x & ~63u);
  if (wbase >= n) return;  // wave-uniform
  const size_t j = wbase + lane;
  bool hit = false;
  if (j < n) {
    uint32_t id[kScIdWords];
    sc_ld_id(id, ids, j);
    hit = sigcache_probe(lines, mask, seed, id);
  }
  const uint64_t hw = __ballot(hit);
  if (lane == 0) hit_words[wbase >> 6] = hw;
}

uint32_t grid_of(uint32_t n) { return (uint32_t)(((size_t)n + kScBlock - 1) / kScBlock); }

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

hipError_t launch_sigcache_probe(const SigCacheDev& c, const uint8_t* ids, const uint8_t* status, uint32_t n,
                                 uint64_t* bitmap, uint32_t* miss_rows, uint32_t* counts,
                                 unsigned long long* counters, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!aligned(c.lines, 128) || !aligned(ids, 16) || !miss_rows || !counts) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sigcache_probe_kernel, dim3(grid_of(n)), dim3(kScBlock), 0, stream, c.lines, c.mask, c.seed, ids,
                     status, n, bitmap, miss_rows, counts, counters);
  return hipGetLastError();
}

hipError_t launch_sigcache_insert(const SigCacheDev& c, const uint32_t* rows, uint32_t m, const uint64_t* cwords,
                                  const uint8_t* ids, hipStream_t stream) {
  if (m == 0) return hipSuccess;
  if (!aligned(c.lines, 128) || !aligned(ids, 16)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sigcache_insert_kernel, dim3(grid_of(m)), dim3(kScBlock), 0, stream, c.lines, c.mask, c.seed,
                     rows, m, cwords, ids);
  return hipGetLastError();
}

hipError_t launch_sigcache_lookup(const SigCacheDev& c, const uint8_t* ids, uint32_t n, uint64_t* hit_words,
                                  hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!aligned(c.lines, 128) || !aligned(ids, 16)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sigcache_lookup_kernel, dim3(grid_of(n)), dim3(kScBlock), 0, stream, c.lines, c.mask, c.seed, ids,
                     n, hit_words);
  return hipGetLastError();
}

}  // namespace stl
