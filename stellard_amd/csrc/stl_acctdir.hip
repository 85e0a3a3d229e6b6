// stl_acctdir.hip -- gfx950 kernels of the account directory (stl_acctdir_*).
// One lane per row, 256-lane workgroups, no LDS.
//
//   acctdir_find_kernel / acctdir_claim_kernel   the two launches of an upsert
//   acctdir_lookup_kernel                        the bare map
//   acctdir_authority_kernel                     Transactor::checkSig's verdict
//                                                per serialized transaction
//
// Visibility.  Per-XCD L2s are not coherent and a CU's L1 is not refreshed by
// other CUs' stores, so the insert is built on a kernel boundary, not on
// fences: in no launch does a lane read anything another workgroup wrote in
// that launch.  find only reads slots, and the ID words of records that
// earlier launches wrote; what it writes (RegularKey and flags of a found
// record, a whole new record past every index a slot names) no lane of the
// launch reads.  claim touches slots with compare-and-swap alone and reads no
// record: the host made the batch's IDs distinct and find already matched
// the ones in the map, so an occupied slot is never this row's ID.  The
// lookups run in later launches and write nothing of the directory.
#include "stl_acctdir.h"

#include "stl_acctdir_core.h"

namespace stl {

namespace {

constexpr uint32_t kAdBlock = 256;  // 4 waves per workgroup

__global__ __launch_bounds__(kAdBlock) void acctdir_find_kernel(const uint32_t* __restrict__ slots,
                                                                uint32_t* records, uint32_t* __restrict__ meta,
                                                                uint32_t mask, uint32_t capacity, uint64_t seed,
                                                                const uint32_t* __restrict__ staged, uint32_t m,
                                                                uint32_t* __restrict__ new_idx) {
  const uint32_t t = blockIdx.x * kAdBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool live = t < m;
  uint32_t w[kAdRecWords];
  uint32_t idx = kAdEmpty;
  if (live) {
    acctdir_load(staged, t, w);
    idx = acctdir_probe(slots, mask, seed, records, w);
    if (idx != kAdEmpty) {
      uint32_t* r = records + (size_t)idx * kAdRecWords;
#pragma unroll
      for (int j = 5; j <= 10; ++j) r[j] = w[j];
    }
  }
  // record indices for the new accounts: one atomic per wave
  const bool fresh = live && idx == kAdEmpty;
  const uint64_t bm = __ballot(fresh);
  uint32_t got = kAdEmpty;
  if (bm != 0) {
    const int leader = __ffsll((unsigned long long)bm) - 1;
    uint32_t b0 = 0;
    if ((int)lane == leader) b0 = atomicAdd(&meta[0], (uint32_t)__popcll(bm));
    b0 = __shfl(b0, leader);
    if (fresh) {
      const uint32_t u = b0 + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
      if (u < capacity) {  // the host refused a batch that does not fit: never false
        uint4* q = reinterpret_cast<uint4*>(records + (size_t)u * kAdRecWords);
        q[0] = make_uint4(w[0], w[1], w[2], w[3]);
        q[1] = make_uint4(w[4], w[5], w[6], w[7]);
        q[2] = make_uint4(w[8], w[9], w[10], 0u);
        got = u;
      }
    }
  }
  if (live) new_idx[t] = got;
}

__global__ __launch_bounds__(kAdBlock) void acctdir_claim_kernel(uint32_t* __restrict__ slots,
                                                                 uint32_t* __restrict__ meta, uint32_t mask,
                                                                 uint64_t seed, const uint32_t* __restrict__ staged,
                                                                 uint32_t m, const uint32_t* __restrict__ new_idx) {
  const uint32_t t = blockIdx.x * kAdBlock + threadIdx.x;
  if (t >= m) return;
  const uint32_t idx = new_idx[t];
  if (idx == kAdEmpty) return;
  uint32_t id[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) id[j] = staged[(size_t)t * kAdRecWords + j];
  uint32_t at = acctdir_hash(id, seed) & mask;
  for (uint32_t p = 0; p <= mask; ++p, at = (at + 1) & mask) {
    if (atomicCAS(&slots[at], kAdEmpty, idx) == kAdEmpty) {
      atomicMax(&meta[1], p + 1);
      return;
    }
  }
}

__global__ __launch_bounds__(kAdBlock) void acctdir_lookup_kernel(const uint32_t* __restrict__ slots,
                                                                  const uint32_t* __restrict__ records, uint32_t mask,
                                                                  uint64_t seed, const uint32_t* __restrict__ account_id,
                                                                  uint32_t n, uint8_t* __restrict__ flags,
                                                                  uint32_t* __restrict__ regular_key) {
  const size_t i = (size_t)blockIdx.x * kAdBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t id[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) id[j] = account_id[5 * i + j];
  const uint32_t idx = acctdir_probe(slots, mask, seed, records, id);
  uint32_t w[kAdRecWords];
#pragma unroll
  for (uint32_t j = 0; j < kAdRecWords; ++j) w[j] = 0u;
  if (idx != kAdEmpty) acctdir_load(records, idx, w);
  const bool there = idx != kAdEmpty && (w[10] & kAcctAbsent) == 0;
  const bool has_key = there && (w[10] & kAcctHasRegularKey) != 0;
  flags[i] = (uint8_t)(there ? w[10] : kAcctNotFound);
  if (regular_key != nullptr) {
    uint32_t* o = regular_key + 5 * i;
#pragma unroll
    for (int j = 0; j < 5; ++j) o[j] = has_key ? w[5 + j] : 0u;
  }
}

__global__ __launch_bounds__(kAdBlock) void acctdir_authority_kernel(
    const uint8_t* __restrict__ blobs, const uint64_t* __restrict__ off, const uint32_t* __restrict__ len, uint32_t n,
    const uint32_t* __restrict__ slots, const uint32_t* __restrict__ records, uint32_t mask, uint64_t seed,
    uint32_t* __restrict__ signer_id, uint32_t* __restrict__ account, uint8_t* __restrict__ authority) {
  const size_t i = (size_t)blockIdx.x * kAdBlock + threadIdx.x;
  if (i >= n) return;
  const uint8_t* b = blobs + off[i];
  const uint32_t L = len[i];
  uint32_t sg[5], ac[5], status;
  const uint32_t auth = acctdir_authority_row(b, b, L, slots, mask, seed, records, sg, ac, &status);
  if (signer_id != nullptr) {
    uint32_t* so = signer_id + 5 * i;
#pragma unroll
    for (int j = 0; j < 5; ++j) so[j] = sg[j];
  }
  if (account != nullptr) {
    uint32_t* ao = account + 5 * i;
#pragma unroll
    for (int j = 0; j < 5; ++j) ao[j] = ac[j];
  }
  authority[i] = (uint8_t)auth;
}

uint32_t grid_of(uint32_t n) { return (uint32_t)(((size_t)n + kAdBlock - 1) / kAdBlock); }

}  // namespace

hipError_t launch_acctdir_find(const AcctDirDev& dir, const uint32_t* staged, uint32_t m, uint32_t* new_idx,
                               hipStream_t stream) {
  if (m == 0) return hipSuccess;
  if (((uintptr_t)staged & 15u) != 0 || ((uintptr_t)dir.records & 15u) != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(acctdir_find_kernel, dim3(grid_of(m)), dim3(kAdBlock), 0, stream, dir.slots, dir.records,
                     dir.meta, dir.mask, dir.capacity, dir.seed, staged, m, new_idx);
  return hipGetLastError();
}

hipError_t launch_acctdir_claim(const AcctDirDev& dir, const uint32_t* staged, uint32_t m, const uint32_t* new_idx,
                                hipStream_t stream) {
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(acctdir_claim_kernel, dim3(grid_of(m)), dim3(kAdBlock), 0, stream, dir.slots, dir.meta,
                     dir.mask, dir.seed, staged, m, new_idx);
  return hipGetLastError();
}

hipError_t launch_acctdir_lookup(const AcctDirDev& dir, const uint8_t* account_id, uint32_t n, uint8_t* flags,
                                 uint8_t* regular_key, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (((uintptr_t)account_id & 3u) != 0 || ((uintptr_t)regular_key & 3u) != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(acctdir_lookup_kernel, dim3(grid_of(n)), dim3(kAdBlock), 0, stream, dir.slots, dir.records,
                     dir.mask, dir.seed, reinterpret_cast<const uint32_t*>(account_id), n, flags,
                     reinterpret_cast<uint32_t*>(regular_key));
  return hipGetLastError();
}

hipError_t launch_acctdir_authority(const AcctDirDev& dir, const uint8_t* blobs, const uint64_t* off,
                                    const uint32_t* len, uint32_t n, uint8_t* signer_id, uint8_t* account,
                                    uint8_t* authority, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (((uintptr_t)signer_id & 3u) != 0 || ((uintptr_t)account & 3u) != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(acctdir_authority_kernel, dim3(grid_of(n)), dim3(kAdBlock), 0, stream, blobs, off, len, n,
                     dir.slots, dir.records, dir.mask, dir.seed, reinterpret_cast<uint32_t*>(signer_id),
                     reinterpret_cast<uint32_t*>(account), authority);
  return hipGetLastError();
}

}  // namespace stl
