// stl_signer.hip -- gfx950 kernels of the signer-authority calls.
//
//   account_id_kernel  one lane per key: two 16-byte loads, Hash160
//                      (stl_hash160.h), five dword stores at byte 20 i -- a
//                      wave's stores cover 1,280 contiguous bytes, and row
//                      n - 1 ends exactly at byte 20 n.
//   tx_signer_kernel   one lane per serialized transaction: the canonical-form
//                      pass (stl_txblob.h) over the blob's bytes in global
//                      memory, then Hash160 of the signing key against the
//                      Account field (stl_signer_core.h).  No atomics, no
//                      workspace.
#include "stl_signer.h"

#include "stl_signer_core.h"

namespace stl {

namespace {

constexpr uint32_t kSgBlock = 256;  // 4 waves per workgroup

__global__ __launch_bounds__(kSgBlock) void account_id_kernel(const uint8_t* __restrict__ pk, uint32_t n,
                                                              uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kSgBlock + threadIdx.x;
  if (i >= n) return;
  const uint4* q = reinterpret_cast<const uint4*>(pk + 32 * i);
  const uint4 a = q[0], b = q[1];
  const uint32_t k[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t h[5];
  hash160_32(k, h);
  uint32_t* o = out + 5 * i;
#pragma unroll
  for (int j = 0; j < 5; ++j) o[j] = h[j];
}

__global__ __launch_bounds__(kSgBlock) void tx_signer_kernel(const uint8_t* __restrict__ blobs,
                                                             const uint64_t* __restrict__ off,
                                                             const uint32_t* __restrict__ len, uint32_t n,
                                                             uint32_t* __restrict__ signer_id,
                                                             uint32_t* __restrict__ account,
                                                             uint8_t* __restrict__ authority) {
  const size_t i = (size_t)blockIdx.x * kSgBlock + threadIdx.x;
  if (i >= n) return;
  const uint8_t* b = blobs + off[i];
  const uint32_t L = len[i];
  uint32_t sg[5], ac[5], status;
  const uint32_t auth = tx_signer_row(b, b, L, sg, ac, &status);
  uint32_t* so = signer_id + 5 * i;
#pragma unroll
  for (int j = 0; j < 5; ++j) so[j] = sg[j];
  if (account != nullptr) {
    uint32_t* ao = account + 5 * i;
#pragma unroll
    for (int j = 0; j < 5; ++j) ao[j] = ac[j];
  }
  authority[i] = (uint8_t)auth;
}

}  // namespace

hipError_t launch_account_id(const uint8_t* pk, uint32_t n, uint8_t* account_id, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (((uintptr_t)pk & 15u) != 0 || ((uintptr_t)account_id & 3u) != 0) return hipErrorInvalidValue;
  const uint32_t grid = (uint32_t)(((size_t)n + kSgBlock - 1) / kSgBlock);
  hipLaunchKernelGGL(account_id_kernel, dim3(grid), dim3(kSgBlock), 0, stream, pk, n,
                     reinterpret_cast<uint32_t*>(account_id));
  return hipGetLastError();
}

hipError_t launch_tx_signer(const uint8_t* blobs, const uint64_t* off, const uint32_t* len, uint32_t n,
                            uint8_t* signer_id, uint8_t* account, uint8_t* authority, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (((uintptr_t)signer_id & 3u) != 0 || ((uintptr_t)account & 3u) != 0) return hipErrorInvalidValue;
  const uint32_t grid = (uint32_t)(((size_t)n + kSgBlock - 1) / kSgBlock);
  hipLaunchKernelGGL(tx_signer_kernel, dim3(grid), dim3(kSgBlock), 0, stream, blobs, off, len, n,
                     reinterpret_cast<uint32_t*>(signer_id), reinterpret_cast<uint32_t*>(account), authority);
  return hipGetLastError();
}

}  // namespace stl
