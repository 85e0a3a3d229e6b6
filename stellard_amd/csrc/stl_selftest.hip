// stl_selftest.hip -- gfx950 kernels of the arithmetic self-test (TEST HOOK:
// stl_debug_selftest_ops_device, stl_debug_selftest_group_device).  They run
// the functions of stl_fe25519.h, stl_sc25519.h, stl_lattice.h, stl_ge25519.h
// and stl_group.h as the device compiles them -- the fenced mad chains, the
// rcp quotient estimate, the wave-wide Lehmer loops, the DPP lane groups --
// on caller-supplied rows, so tests can compare every output word with the
// host build of the same source (row formats: stl_selftest.h).
//
//   selftest_ops_kernel    one lane per row; the whole op sits under the
//                          row < n guard (lattice_half's wave votes included:
//                          the active lanes of the last wave vote among
//                          themselves).
//   selftest_group_kernel  one group of G lanes per row, role bits from the
//                          lane index as verify_main_group_kernel takes them.
//                          The grid is whole waves and lanes past the last
//                          row rerun the last row, so no DPP source lane is
//                          ever inactive; they store nothing.
#include "stl_kernels.h"

#include "../../include/stl.h"
#include "stl_group.h"
#include "stl_selftest.h"

namespace stl {

static_assert(kSelftestOps == STL_SELFTEST_OPS && kSelftestGroupOps == STL_SELFTEST_GROUP_OPS, "stl.h op counts");
static_assert(kSelftestInWords == STL_SELFTEST_IN_WORDS && kSelftestOutWords == STL_SELFTEST_OUT_WORDS,
              "stl.h row sizes");

namespace {

constexpr uint32_t kStBlock = 64;  // one wave per workgroup

__global__ __launch_bounds__(kStBlock) void selftest_ops_kernel(uint32_t op, const uint32_t* __restrict__ in,
                                                                uint32_t n, uint32_t* __restrict__ out) {
  const size_t row = (size_t)blockIdx.x * kStBlock + threadIdx.x;
  if (row < n) {
    uint32_t r[kSelftestInWords], o[kSelftestOutWords];
    const uint32_t* src = in + row * kSelftestInWords;
#pragma unroll
    for (int i = 0; i < kSelftestInWords; ++i) r[i] = src[i];
    selftest_op(op, r, o);
    uint32_t* dst = out + row * kSelftestOutWords;
#pragma unroll
    for (int i = 0; i < kSelftestOutWords; ++i) dst[i] = o[i];
  }
}

template <int G>
__global__ __launch_bounds__(kStBlock) void selftest_group_kernel(uint32_t op, const uint32_t* __restrict__ in,
                                                                  uint32_t nrows, uint32_t* __restrict__ out) {
  static_assert(G == 2 || G == 4, "group size");
  const size_t gl = (size_t)blockIdx.x * kStBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const GroupRole q{(lane & 1u) != 0, (lane & 2u) != 0};
  const bool live = gl / G < nrows;
  const size_t row = live ? gl / G : nrows - 1;
  const uint32_t* src = in + row * kSelftestInWords;
  fe f[8], o[4];
#pragma unroll
  for (int j = 0; j < 8; ++j) selftest_ld(f[j], src, j);
#pragma unroll
  for (int j = 0; j < 4; ++j) fe_0(o[j]);
  switch (op) {  // wave-uniform
    case kGrpMul4:
      group_mul4<G>(o, f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], q);
      break;
    case kGrpSq4:
      group_sq4<G>(o, f[0], f[1], f[2], f[3], q);
      break;
    case kGrpP2Dbl: {
      const ge_p2 p{f[0], f[1], f[2]};
      ge_p1p1 r;
      group_p2_dbl<G>(r, p, q);
      o[0] = r.X;
      o[1] = r.Y;
      o[2] = r.Z;
      o[3] = r.T;
      break;
    }
    case kGrpToP3: {
      const ge_p1p1 t{f[0], f[1], f[2], f[3]};
      ge_p3 r;
      group_to_p3<G>(r, t, q);
      o[0] = r.X;
      o[1] = r.Y;
      o[2] = r.Z;
      o[3] = r.T;
      break;
    }
    case kGrpToP2: {
      const ge_p1p1 t{f[0], f[1], f[2], f[3]};
      ge_p2 r;
      group_to_p2<G>(r, t, q);
      o[0] = r.X;
      o[1] = r.Y;
      o[2] = r.Z;
      break;
    }
    case kGrpAddCached: {
      const ge_p3 p{f[0], f[1], f[2], f[3]};
      const ge_cached c{f[4], f[5], f[6], f[7]};
      ge_p1p1 r;
      group_add_cached<G>(r, p, c, q);
      o[0] = r.X;
      o[1] = r.Y;
      o[2] = r.Z;
      o[3] = r.T;
      break;
    }
    case kGrpMadd: {
      const ge_p3 p{f[0], f[1], f[2], f[3]};
      const ge_niels n{f[4], f[5], f[6]};
      ge_p1p1 r;
      group_madd<G>(r, p, n, q);
      o[0] = r.X;
      o[1] = r.Y;
      o[2] = r.Z;
      o[3] = r.T;
      break;
    }
    default:
      break;
  }
  if (live) {
    uint32_t* dst = out + gl * kSelftestOutWords;
#pragma unroll
    for (int j = 0; j < 4; ++j) selftest_st(dst, j, o[j]);
#pragma unroll
    for (int i = kSelftestFlagWord; i < kSelftestOutWords; ++i) dst[i] = 0;
  }
}

}  // namespace

hipError_t launch_selftest_ops(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t stream) {
  if (op >= kSelftestOps) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)(((size_t)n + kStBlock - 1) / kStBlock);
  hipLaunchKernelGGL(selftest_ops_kernel, dim3(grid), dim3(kStBlock), 0, stream, op, in, n, out);
  return hipGetLastError();
}

hipError_t launch_selftest_group(uint32_t op, uint32_t G, const uint32_t* in, uint32_t nrows, uint32_t* out,
                                 hipStream_t stream) {
  if (op >= kSelftestGroupOps || (G != 2 && G != 4)) return hipErrorInvalidValue;
  if (nrows == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)(((size_t)nrows * G + kStBlock - 1) / kStBlock);  // whole waves
  if (G == 4)
    hipLaunchKernelGGL(selftest_group_kernel<4>, dim3(grid), dim3(kStBlock), 0, stream, op, in, nrows, out);
  else
    hipLaunchKernelGGL(selftest_group_kernel<2>, dim3(grid), dim3(kStBlock), 0, stream, op, in, nrows, out);
  return hipGetLastError();
}

}  // namespace stl
