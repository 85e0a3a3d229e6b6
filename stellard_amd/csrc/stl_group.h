// stl_group.h -- device only: the lane-group forms of the group formulas
// (verify_main_group_kernel, stl_kernels.hip) and the DPP moves under them, in
// a header of their own so that the arithmetic self-test (stl_selftest.hip)
// runs the very functions the product kernels run.
#pragma once
#include "stl_ge25519.h"

namespace stl {

// The value of the other lane of this lane's pair (lane ^ 1): one DPP move,
// quad_perm [1,0,3,2] (dpp_ctrl 0xB1), a register-to-register swap inside the
// VALU -- __shfl_xor lowers to ds_bpermute_b32, an LDS round trip per value.
__device__ __forceinline__ uint32_t pair_swap(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
}

// ---- lane groups per chain: the smallest batches (verify_main_group_kernel) ----
// A chunk this small leaves most SIMDs idle, so its time is one lane's
// dependent chain, which a lone wave issues at about one mad64 per 5.8 cycles.
// Here the four products of each group formula (the squarings of a doubling,
// the products of an addition or of a conversion) are spread over a group of
// G lanes -- G = 4 (a quad: one product per lane, four DPP quad broadcasts)
// or G = 2 (a duo: two interleaved products per lane, one DPP pair swap) --
// and every lane then holds the whole point again.  Role bits b0 = lane & 1,
// b1 = lane & 2.
struct GroupRole {
  bool b0, b1;
};

template <int S>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, S | (S << 2) | (S << 4) | (S << 6), 0xF, 0xF, false);
}

__device__ __forceinline__ void fe_sel2(fe& o, const fe& a0, const fe& a1, bool b) {
#pragma unroll
  for (int i = 0; i < 9; ++i) o.v[i] = b ? a1.v[i] : a0.v[i];
}

// o = [a0, a1, a2, a3][role]
__device__ __forceinline__ void fe_sel4(fe& o, const fe& a0, const fe& a1, const fe& a2, const fe& a3, GroupRole r) {
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const uint32_t lo = r.b0 ? a1.v[i] : a0.v[i];
    const uint32_t hi = r.b0 ? a3.v[i] : a2.v[i];
    o.v[i] = r.b1 ? hi : lo;
  }
}

__device__ __forceinline__ void quad_gather(fe out[4], const fe& p) {
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    out[0].v[i] = quad_bcast<0>(p.v[i]);
    out[1].v[i] = quad_bcast<1>(p.v[i]);
    out[2].v[i] = quad_bcast<2>(p.v[i]);
    out[3].v[i] = quad_bcast<3>(p.v[i]);
  }
}

// duo: this lane's products p0, p1 are products 2*b0 and 2*b0 + 1
__device__ __forceinline__ void duo_gather(fe out[4], const fe& p0, const fe& p1, bool b0) {
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const uint32_t q0 = pair_swap(p0.v[i]), q1 = pair_swap(p1.v[i]);
    out[0].v[i] = b0 ? q0 : p0.v[i];
    out[1].v[i] = b0 ? q1 : p1.v[i];
    out[2].v[i] = b0 ? p0.v[i] : q0;
    out[3].v[i] = b0 ? p1.v[i] : q1;
  }
}

// out[j] = a_j * b_j on every lane of the group (same bounds as fe_mul)
template <int G>
__device__ __forceinline__ void group_mul4(fe out[4], const fe& a0, const fe& b0, const fe& a1, const fe& b1,
                                           const fe& a2, const fe& b2, const fe& a3, const fe& b3, GroupRole r) {
  if (G == 4) {
    fe a, b, p;
    fe_sel4(a, a0, a1, a2, a3, r);
    fe_sel4(b, b0, b1, b2, b3, r);
    fe_mul(p, a, b);
    quad_gather(out, p);
  } else {
    fe x0, y0, x1, y1, p0, p1;
    fe_sel2(x0, a0, a2, r.b0);
    fe_sel2(y0, b0, b2, r.b0);
    fe_sel2(x1, a1, a3, r.b0);
    fe_sel2(y1, b1, b3, r.b0);
    fe_mul2(p0, x0, y0, p1, x1, y1);
    duo_gather(out, p0, p1, r.b0);
  }
}

template <int G>
__device__ __forceinline__ void group_sq4(fe out[4], const fe& a0, const fe& a1, const fe& a2, const fe& a3,
                                          GroupRole r) {
  if (G == 4) {
    fe a, p;
    fe_sel4(a, a0, a1, a2, a3, r);
    fe_sq(p, a);
    quad_gather(out, p);
  } else {
    fe x0, x1, p0, p1;
    fe_sel2(x0, a0, a2, r.b0);
    fe_sel2(x1, a1, a3, r.b0);
    fe_sq2(p0, x0, p1, x1);
    duo_gather(out, p0, p1, r.b0);
  }
}

// ge_p2_dbl (non-lazy X): the four squarings spread over the group
template <int G>
__device__ __forceinline__ void group_p2_dbl(ge_p1p1& r, const ge_p2& p, GroupRole q) {
  fe XpY, S[4];
  fe_add(XpY, p.X, p.Y);     // [2]
  group_sq4<G>(S, p.X, p.Y, p.Z, XpY, q);  // XX, YY, Z^2, A
  fe ZZ2;
  fe_add(ZZ2, S[2], S[2]);   // [2]
  fe_add(r.Y, S[1], S[0]);   // [2]
  fe_sub_nc<2>(r.Z, S[1], S[0]);  // [3]
  fe_sub(r.X, S[3], r.Y);    // [1]
  fe_sub(r.T, ZZ2, r.Z);     // [1]
}

// ge_p1p1_to_p3 (the p2 conversion is its first three products)
template <int G>
__device__ __forceinline__ void group_to_p3(ge_p3& r, const ge_p1p1& t, GroupRole q) {
  fe O[4];
  group_mul4<G>(O, t.X, t.T, t.Y, t.Z, t.Z, t.T, t.X, t.Y, q);
  r.X = O[0];
  r.Y = O[1];
  r.Z = O[2];
  r.T = O[3];
}

template <int G>
__device__ __forceinline__ void group_to_p2(ge_p2& r, const ge_p1p1& t, GroupRole q) {
  ge_p3 p;
  group_to_p3<G>(p, t, q);
  r.X = p.X;
  r.Y = p.Y;
  r.Z = p.Z;
}

// ge_add_cached
template <int G>
__device__ __forceinline__ void group_add_cached(ge_p1p1& r, const ge_p3& p, const ge_cached& c, GroupRole q) {
  fe t, t2, O[4];
  fe_sub_nc<2>(t, p.Y, p.X);  // [3]
  fe_add(t2, p.Y, p.X);       // [2]
  group_mul4<G>(O, t, c.YmX, t2, c.YpX, c.T2d, p.T, p.Z, c.Z, q);
  fe D;
  fe_add(D, O[3], O[3]);      // [2]
  fe_sub_nc<2>(r.X, O[1], O[0]);  // [3]
  fe_add(r.Y, O[1], O[0]);    // [2]
  fe_add(r.Z, D, O[2]);       // [3]
  fe_sub(r.T, D, O[2]);       // [1]
}

// ge_madd (the fourth product is not used)
template <int G>
__device__ __forceinline__ void group_madd(ge_p1p1& r, const ge_p3& p, const ge_niels& n, GroupRole q) {
  fe t, t2, O[4];
  fe_sub_nc<2>(t, p.Y, p.X);  // [3]
  fe_add(t2, p.Y, p.X);       // [2]
  group_mul4<G>(O, t, n.ymx, t2, n.ypx, n.xy2d, p.T, p.Z, p.Z, q);
  fe D;
  fe_add(D, p.Z, p.Z);        // [2]
  fe_sub_nc<2>(r.X, O[1], O[0]);  // [3]
  fe_add(r.Y, O[1], O[0]);    // [2]
  fe_add(r.Z, D, O[2]);       // [3]
  fe_sub(r.T, D, O[2]);       // [1]
}

}  // namespace stl
