// stl_keyset.hip -- gfx950 kernels of the registered signer sets (stl_keyset_*).
//
//   keyset_decode_kernel  registration: one lane per key -- decode, flags,
//                         the key's record (stl_comb.h).
//   keyset_build_kernel   registration: one lane per (key, window) -- the
//                         window base by doubling, its 128 multiples by
//                         additions, one inversion for the 128 rows.
//   keyset_verify_kernel  one signature per lane: k = SHA-512(R || A || M) mod L
//                         with A from the key's record, 64 additions of table
//                         rows, encode, compare with R; accept bits per wave
//                         with a 64-bit ballot.
//   keyset_lookup_kernel        verify by public key: one lane per row, the
//                               key's index through the map (stl_keyset_map.h)
//                               and the list of the rows that have none.
//   keyset_gather_rows_kernel   those rows' signature, message and key into
//                               compact arrays for the per-signature kernels.
//   keyset_scatter_bits_kernel  their accept bits back into the call's bitmap.
#include "stl_keyset.h"

#include "stl_comb.h"
#include "stl_keyset_map.h"

namespace stl {

namespace {

constexpr uint32_t kKsBlock = 256;      // verify: 4 waves per workgroup
constexpr uint32_t kKsBuildBlock = 64;  // build: one wave, so a few keys already fill the chip

__device__ __forceinline__ void ks_ld8(uint32_t w[8], const uint8_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

__global__ __launch_bounds__(kKsBuildBlock) void keyset_decode_kernel(const uint8_t* __restrict__ pk, uint32_t nkeys,
                                                                      uint32_t* __restrict__ rec) {
  const uint32_t t = blockIdx.x * kKsBuildBlock + threadIdx.x;
  if (t > nkeys) return;  // record nkeys is the base point's
  uint32_t A[8], r[kKeyRecWords];
  ks_ld8(A, pk + 32 * (size_t)t);
  comb_key_record(r, A, t == nkeys);
  uint4* q = reinterpret_cast<uint4*>(rec + (size_t)t * kKeyRecWords);
#pragma unroll
  for (int i = 0; i < kKeyRecWords / 4; ++i) q[i] = make_uint4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
}

__global__ __launch_bounds__(kKsBuildBlock) void keyset_build_kernel(const uint32_t* __restrict__ rec, uint32_t first,
                                                                     uint32_t count, uint32_t* __restrict__ tables,
                                                                     uint32_t* __restrict__ scratch) {
  const uint32_t t = blockIdx.x * kKsBuildBlock + threadIdx.x;
  if (t >= count * (uint32_t)kCombWindows) return;
  const uint32_t key = first + t / kCombWindows, w = t % kCombWindows;
  const uint32_t* r = rec + (size_t)key * kKeyRecWords;
  if (!(r[kKeyRecFlags] & kKeyDecodes)) return;  // no rows
  uint32_t rr[kKeyRecWords];
#pragma unroll
  for (int i = 0; i < kKeyRecWords; ++i) rr[i] = r[i];
  ge_p3 P, W;
  comb_record_point(P, rr);
  comb_window_base(W, P, (int)w);
  comb_build_window(tables + (size_t)key * kCombKeyWords + (size_t)w * kCombRows * kCombRowWords,
                    scratch + (size_t)t * kCombScratchWords, W);
}

__global__ __launch_bounds__(kKsBlock, 2) void keyset_verify_kernel(
    const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg, const uint32_t* __restrict__ key_index,
    uint32_t n, const uint32_t* __restrict__ rec, const uint32_t* __restrict__ tables, uint32_t nkeys,
    uint32_t policy, uint64_t* __restrict__ bitmap, unsigned long long* __restrict__ ctr) {
  const uint32_t lane = threadIdx.x & 63u;
  const size_t wbase = (size_t)blockIdx.x * kKsBlock + (threadIdx.x & ~63u);
  if (wbase >= n) return;  // wave-uniform
  const size_t j = wbase + lane;
  bool ok = false;
  if (j < n) {
    const uint32_t ki = key_index[j];
    if (ki < nkeys) {
      uint32_t R[8], S[8], A[8], M[8], h[16], k[8];
      ks_ld8(R, sig + 64 * j);
      ks_ld8(S, sig + 64 * j + 32);
      ks_ld8(M, msg + 32 * j);
      const uint32_t* r = rec + (size_t)ki * kKeyRecWords;
      ks_ld8(A, reinterpret_cast<const uint8_t*>(r));
      const uint32_t kflags = r[kKeyRecFlags];
      sha512_hram32(h, R, A, M);
      sc_reduce64(k, h);
      ok = verify_comb_with_k(R, S, kflags, k, policy, tables + (size_t)ki * kCombKeyWords,
                              tables + (size_t)nkeys * kCombKeyWords);
    }
  }
  const uint64_t word = __ballot(ok);
  if (lane == 0) {
    bitmap[wbase >> 6] = word;
    if (ctr) atomicAdd(&ctr[0], (unsigned long long)__popcll(word));  // accepted (stl_get_stats)
  }
}

// ---- verify by public key: lookup, and the rows of unregistered signers ----

// One lane per row: the key's index through the map, or kKsMapEmpty.  With a
// miss counter, one ballot per wave gives the wave's misses, lane 0 reserves
// their places with one atomic add, and (with a list) each missing lane
// stores its row number at its rank among them.
__global__ __launch_bounds__(kKsBlock) void keyset_lookup_kernel(
    const uint8_t* __restrict__ pk, uint32_t n, const uint32_t* __restrict__ slots, uint32_t mask, uint32_t max_probe,
    uint64_t seed, const uint32_t* __restrict__ rec, uint32_t* __restrict__ key_index,
    uint32_t* __restrict__ miss_rows, uint32_t* __restrict__ miss_count) {
  const uint32_t lane = threadIdx.x & 63u;
  const size_t wbase = (size_t)blockIdx.x * kKsBlock + (threadIdx.x & ~63u);
  if (wbase >= n) return;  // wave-uniform
  const size_t j = wbase + lane;
  bool miss = false;
  if (j < n) {
    uint32_t A[8];
    ks_ld8(A, pk + 32 * j);
    const uint32_t ki = keyset_map_probe(slots, mask, seed, max_probe, rec, kKeyRecWords, A);
    key_index[j] = ki;
    miss = ki == kKsMapEmpty;
  }
  if (!miss_count) return;
  const uint64_t m = __ballot(miss);
  if (m == 0) return;  // wave-uniform
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(miss_count, (uint32_t)__popcll(m));
  base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
  if (miss && miss_rows) miss_rows[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)j;
}

// Eight lanes per listed row, 16 bytes each: four of the signature, two of
// the message, two of the key.
__global__ __launch_bounds__(kKsBlock) void keyset_gather_rows_kernel(
    const uint32_t* __restrict__ rows, uint32_t m, const uint4* __restrict__ sig, const uint4* __restrict__ msg,
    const uint4* __restrict__ pk, uint4* __restrict__ csig, uint4* __restrict__ cmsg, uint4* __restrict__ cpk) {
  const size_t t = (size_t)blockIdx.x * kKsBlock + threadIdx.x;
  const size_t j = t >> 3;
  if (j >= m) return;
  const uint32_t p = (uint32_t)t & 7u;
  const size_t r = rows[j];
  if (p < 4) csig[4 * j + p] = sig[4 * r + p];
  else if (p < 6) cmsg[2 * j + (p - 4)] = msg[2 * r + (p - 4)];
  else cpk[2 * j + (p - 6)] = pk[2 * r + (p - 6)];
}

// One lane per listed row: its accept bit, if set, into the caller's bitmap
// (whose word holds 0 for the row: keyset_verify_kernel wrote it).
__global__ __launch_bounds__(kKsBlock) void keyset_scatter_bits_kernel(const uint32_t* __restrict__ rows, uint32_t m,
                                                                       const uint64_t* __restrict__ cwords,
                                                                       uint64_t* __restrict__ bitmap) {
  const size_t j = (size_t)blockIdx.x * kKsBlock + threadIdx.x;
  if (j >= m) return;
  if (!((cwords[j >> 6] >> (j & 63u)) & 1ull)) return;
  const uint32_t r = rows[j];
  atomicOr(reinterpret_cast<unsigned long long*>(bitmap) + (r >> 6), 1ull << (r & 63u));
}

}  // namespace

KeysetGeometry keyset_geometry() {
  return KeysetGeometry{(uint32_t)kCombBits, (uint32_t)kCombWindows, (uint32_t)kCombRows, (uint32_t)kCombRowWords * 4u};
}
size_t keyset_key_words() { return kCombKeyWords; }
size_t keyset_rec_words() { return kKeyRecWords; }
size_t keyset_scratch_words_per_key() { return (size_t)kCombWindows * kCombScratchWords; }

hipError_t launch_keyset_decode(const uint8_t* d_pk, uint32_t nkeys, uint32_t* rec, hipStream_t stream) {
  const uint32_t grid = (nkeys + 1 + kKsBuildBlock - 1) / kKsBuildBlock;
  hipLaunchKernelGGL(keyset_decode_kernel, dim3(grid), dim3(kKsBuildBlock), 0, stream, d_pk, nkeys, rec);
  return hipGetLastError();
}

hipError_t launch_keyset_build(const uint32_t* rec, uint32_t first, uint32_t count, uint32_t* tables,
                               uint32_t* scratch, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  const uint32_t grid = (count * (uint32_t)kCombWindows + kKsBuildBlock - 1) / kKsBuildBlock;
  hipLaunchKernelGGL(keyset_build_kernel, dim3(grid), dim3(kKsBuildBlock), 0, stream, rec, first, count, tables,
                     scratch);
  return hipGetLastError();
}

hipError_t launch_keyset_verify(const uint8_t* sig, const uint8_t* msg, const uint32_t* key_index, uint32_t n,
                                const uint32_t* rec, const uint32_t* tables, uint32_t nkeys, uint32_t policy,
                                uint64_t* bitmap, unsigned long long* counters, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)(((size_t)n + kKsBlock - 1) / kKsBlock);
  hipLaunchKernelGGL(keyset_verify_kernel, dim3(grid), dim3(kKsBlock), 0, stream, sig, msg, key_index, n, rec, tables,
                     nkeys, policy, bitmap, counters);
  return hipGetLastError();
}

hipError_t launch_keyset_lookup(const uint8_t* pk, uint32_t n, const KeysetMapDev& map, const uint32_t* rec,
                                uint32_t* key_index, uint32_t* miss_rows, uint32_t* miss_count,
                                hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (miss_rows && !miss_count) return hipErrorInvalidValue;
  const uint32_t grid = (uint32_t)(((size_t)n + kKsBlock - 1) / kKsBlock);
  hipLaunchKernelGGL(keyset_lookup_kernel, dim3(grid), dim3(kKsBlock), 0, stream, pk, n, map.slots, map.mask,
                     map.max_probe, map.seed, rec, key_index, miss_rows, miss_count);
  return hipGetLastError();
}

hipError_t launch_keyset_gather_rows(const uint32_t* rows, uint32_t m, const uint8_t* sig, const uint8_t* msg,
                                     const uint8_t* pk, uint8_t* csig, uint8_t* cmsg, uint8_t* cpk,
                                     hipStream_t stream) {
  if (m == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)(((size_t)m * 8 + kKsBlock - 1) / kKsBlock);
  hipLaunchKernelGGL(keyset_gather_rows_kernel, dim3(grid), dim3(kKsBlock), 0, stream, rows, m,
                     reinterpret_cast<const uint4*>(sig), reinterpret_cast<const uint4*>(msg),
                     reinterpret_cast<const uint4*>(pk), reinterpret_cast<uint4*>(csig),
                     reinterpret_cast<uint4*>(cmsg), reinterpret_cast<uint4*>(cpk));
  return hipGetLastError();
}

hipError_t launch_keyset_scatter_bits(const uint32_t* rows, uint32_t m, const uint64_t* cwords, uint64_t* bitmap,
                                      hipStream_t stream) {
  if (m == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)(((size_t)m + kKsBlock - 1) / kKsBlock);
  hipLaunchKernelGGL(keyset_scatter_bits_kernel, dim3(grid), dim3(kKsBlock), 0, stream, rows, m, cwords, bitmap);
  return hipGetLastError();
}

}  // namespace stl
