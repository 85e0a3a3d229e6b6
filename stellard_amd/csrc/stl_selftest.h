// stl_selftest.h -- TEST HOOK: one op table over the field, scalar and group
// arithmetic, shared by the host harness (tests/native/hostemu.cpp,
// hostemu_selftest_ops) and the device (stl_selftest.hip,
// stl_debug_selftest_ops_device), so each function of stl_fe25519.h,
// stl_sc25519.h, stl_lattice.h and stl_ge25519.h can be checked on its own --
// against Python integers on the host, and word for word host against gfx950.
// No verify path calls anything in this file.
//
// Row format (32-bit words, raw: nothing is reduced on the way in and nothing
// is canonicalised on the way out, except where the op itself is fe_tobytes):
//
//   input row   kSelftestInWords = 72 words: eight slots of nine words.  A
//               field element occupies one slot, limb i in word i of the slot
//               (fe f_j = words 9j .. 9j+8).  Scalar ops read plain
//               little-endian words from word 0 on, as listed per op.  A
//               flag or count an op takes next to its field elements is word
//               0 of the first slot those do not use.
//   output row  kSelftestOutWords = 40 words: four slots of nine words (field
//               elements, or scalar / byte words from word 0 on) and four flag
//               words 36..39.  Every word an op does not write is 0.
//
// Per op (f_j input slots, o_j output slots, w[] input words, F_j flag words):
//   field   fe_mul o0 = f0*f1; fe_sq o0 = f0^2; fe_mul2 o_j = f_2j*f_2j+1
//           (j < 2); fe_mul3 (j < 3); fe_mul4 (j < 4); fe_sq2 o_j = f_j^2
//           (j < 2); fe_sq4 (j < 4); fe_sq_n<3> (j < 3); fe_sqn o0 =
//           f0^(2^n), n = w[9] & 63; fe_add / fe_sub / fe_sub_nc<2> /
//           fe_sub_nc<3> o0 = f0 op f1; fe_neg / fe_neg_nc<2> / fe_carry o0 =
//           op(f0); fe_cmov o0 = w[18] ? f1 : f0; fe_frombytes o0 =
//           limbs(w[0..7]); fe_tobytes out[0..7] = bytes(f0); fe_iszero /
//           fe_isnegative F0; fe_invert / fe_pow22523 o0 = op(f0);
//           fe_const_* o0.
//   scalar  sc_reduce64 out[0..7] = w[0..15] mod L; sc_muladd out[0..7] =
//           w[0..7]*w[8..15] + w[16..23] mod L; sc_lt_L F0; sc_recode16 /
//           256 / 65536 out[0..7] = packed digits of w[0..7]; sc_mul_signed
//           out[0..7] = (w[5] ? -1 : 1) * w[0..4] * w[8..15] mod L;
//           lattice_half out[0..4] = |c|, out[5..9] = |d| for k = w[0..7],
//           F0 = ok, F1 = c < 0, F2 = d < 0; sc_recode16_half out[0..4] =
//           packed digits of w[0..4], F0 = positions needed.
//   group   points take consecutive slots in the order of their struct
//           (p2 X Y Z; p3 / p1p1 X Y Z T; cached YpX YmX Z T2d; niels ypx ymx
//           xy2d), outputs likewise from o0.  ge_p2_dbl<false / true> (f0..2),
//           ge_affine_dbl (p3 f0..3), ge_add_cached (p3 f0..3, cached f4..7),
//           ge_madd (p3 f0..3, niels f4..6), ge_p1p1_to_p2 / _p3 (f0..3),
//           ge_p3_to_cached (f0..3), ge_cached_cneg (f0..3, neg = w[36]),
//           ge_niels_cneg (f0..2, neg = w[27]), ge_frombytes_negate_vartime
//           (s = w[0..7]; o0..3 = point, F0 = ok), ge_tobytes (p2 f0..2;
//           out[0..7]).
//
// The lane-group ops (kGrp*, device only: stl_group.h) take the rows of the
// one-lane op they restate: group_mul4 / group_sq4 as fe_mul4 / fe_sq4,
// group_p2_dbl as ge_p2_dbl<false>, group_to_p3 / group_to_p2 as
// ge_p1p1_to_p3 (group_to_p2 leaves o3 zero), group_add_cached as
// ge_add_cached, group_madd as ge_madd.
#pragma once
#include "stl_ge25519.h"
#include "stl_lattice.h"

namespace stl {

constexpr int kSelftestInWords = 72;
constexpr int kSelftestOutWords = 40;
constexpr int kSelftestFlagWord = 36;

// The op codes, in the order tests/arith_cases.py reads them from this file.
enum SelftestOp : uint32_t {
  kOpFeMul = 0,
  kOpFeSq,
  kOpFeMul2,
  kOpFeSq2,
  kOpFeMul3,
  kOpFeMul4,
  kOpFeSq4,
  kOpFeSqN3,
  kOpFeSqn,
  kOpFeAdd,
  kOpFeSub,
  kOpFeNeg,
  kOpFeSubNc2,
  kOpFeSubNc3,
  kOpFeNegNc2,
  kOpFeCarry,
  kOpFeCmov,
  kOpFeFrombytes,
  kOpFeTobytes,
  kOpFeIszero,
  kOpFeIsnegative,
  kOpFeInvert,
  kOpFePow22523,
  kOpFeConstD,
  kOpFeConst2d,
  kOpFeConstSqrtm1,
  kOpScReduce64,
  kOpScMuladd,
  kOpScLtL,
  kOpScRecode16,
  kOpScRecode256,
  kOpScRecode65536,
  kOpScMulSigned,
  kOpLatticeHalf,
  kOpScRecode16Half,
  kOpGeP2Dbl,
  kOpGeP2DblLazy,
  kOpGeAffineDbl,
  kOpGeAddCached,
  kOpGeMadd,
  kOpGeP1p1ToP2,
  kOpGeP1p1ToP3,
  kOpGeP3ToCached,
  kOpGeCachedCneg,
  kOpGeNielsCneg,
  kOpGeFrombytesNegate,
  kOpGeTobytes,
  kSelftestOps
};

enum SelftestGroupOp : uint32_t {
  kGrpMul4 = 0,
  kGrpSq4,
  kGrpP2Dbl,
  kGrpToP3,
  kGrpToP2,
  kGrpAddCached,
  kGrpMadd,
  kSelftestGroupOps
};

STL_HD void selftest_ld(fe& f, const uint32_t* in, int slot) {
#pragma unroll
  for (int i = 0; i < 9; ++i) f.v[i] = in[9 * slot + i];
}

STL_HD void selftest_st(uint32_t* out, int slot, const fe& f) {
#pragma unroll
  for (int i = 0; i < 9; ++i) out[9 * slot + i] = f.v[i];
}

STL_HD void selftest_ld_p3(ge_p3& p, const uint32_t* in) {
  selftest_ld(p.X, in, 0);
  selftest_ld(p.Y, in, 1);
  selftest_ld(p.Z, in, 2);
  selftest_ld(p.T, in, 3);
}

STL_HD void selftest_ld_p1p1(ge_p1p1& p, const uint32_t* in) {
  selftest_ld(p.X, in, 0);
  selftest_ld(p.Y, in, 1);
  selftest_ld(p.Z, in, 2);
  selftest_ld(p.T, in, 3);
}

STL_HD void selftest_ld_p2(ge_p2& p, const uint32_t* in) {
  selftest_ld(p.X, in, 0);
  selftest_ld(p.Y, in, 1);
  selftest_ld(p.Z, in, 2);
}

STL_HD void selftest_ld_cached(ge_cached& c, const uint32_t* in, int slot) {
  selftest_ld(c.YpX, in, slot);
  selftest_ld(c.YmX, in, slot + 1);
  selftest_ld(c.Z, in, slot + 2);
  selftest_ld(c.T2d, in, slot + 3);
}

STL_HD void selftest_ld_niels(ge_niels& n, const uint32_t* in, int slot) {
  selftest_ld(n.ypx, in, slot);
  selftest_ld(n.ymx, in, slot + 1);
  selftest_ld(n.xy2d, in, slot + 2);
}

STL_HD void selftest_st_p1p1(uint32_t* out, const ge_p1p1& r) {
  selftest_st(out, 0, r.X);
  selftest_st(out, 1, r.Y);
  selftest_st(out, 2, r.Z);
  selftest_st(out, 3, r.T);
}

STL_HD void selftest_st_p3(uint32_t* out, const ge_p3& r) {
  selftest_st(out, 0, r.X);
  selftest_st(out, 1, r.Y);
  selftest_st(out, 2, r.Z);
  selftest_st(out, 3, r.T);
}

// Runs op on one input row (kSelftestInWords words) and writes one output
// row (kSelftestOutWords words).  An op code >= kSelftestOps leaves the row
// zero (the entry points refuse it before any row runs).
STL_HD void selftest_op(uint32_t op, const uint32_t* in, uint32_t* out) {
#pragma unroll
  for (int i = 0; i < kSelftestOutWords; ++i) out[i] = 0;
  uint32_t* flag = out + kSelftestFlagWord;
  fe f[8], o[4];
  switch (op) {
    case kOpFeMul:
      selftest_ld(f[0], in, 0);
      selftest_ld(f[1], in, 1);
      fe_mul(o[0], f[0], f[1]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeSq:
      selftest_ld(f[0], in, 0);
      fe_sq(o[0], f[0]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeMul2:
#pragma unroll
      for (int j = 0; j < 4; ++j) selftest_ld(f[j], in, j);
      fe_mul2(o[0], f[0], f[1], o[1], f[2], f[3]);
      selftest_st(out, 0, o[0]);
      selftest_st(out, 1, o[1]);
      break;
    case kOpFeSq2:
      selftest_ld(f[0], in, 0);
      selftest_ld(f[1], in, 1);
      fe_sq2(o[0], f[0], o[1], f[1]);
      selftest_st(out, 0, o[0]);
      selftest_st(out, 1, o[1]);
      break;
    case kOpFeMul3:
#pragma unroll
      for (int j = 0; j < 6; ++j) selftest_ld(f[j], in, j);
      fe_mul3(o[0], f[0], f[1], o[1], f[2], f[3], o[2], f[4], f[5]);
#pragma unroll
      for (int j = 0; j < 3; ++j) selftest_st(out, j, o[j]);
      break;
    case kOpFeMul4:
#pragma unroll
      for (int j = 0; j < 8; ++j) selftest_ld(f[j], in, j);
      fe_mul4(o[0], f[0], f[1], o[1], f[2], f[3], o[2], f[4], f[5], o[3], f[6], f[7]);
#pragma unroll
      for (int j = 0; j < 4; ++j) selftest_st(out, j, o[j]);
      break;
    case kOpFeSq4:
#pragma unroll
      for (int j = 0; j < 4; ++j) selftest_ld(f[j], in, j);
      fe_sq4(o[0], f[0], o[1], f[1], o[2], f[2], o[3], f[3]);
#pragma unroll
      for (int j = 0; j < 4; ++j) selftest_st(out, j, o[j]);
      break;
    case kOpFeSqN3: {
#pragma unroll
      for (int j = 0; j < 3; ++j) selftest_ld(f[j], in, j);
      const fe* a[3] = {&f[0], &f[1], &f[2]};
      fe_sq_n<3>(o, a);
#pragma unroll
      for (int j = 0; j < 3; ++j) selftest_st(out, j, o[j]);
      break;
    }
    case kOpFeSqn:
      selftest_ld(f[0], in, 0);
      fe_sqn(o[0], f[0], (int)(in[9] & 63u));
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeAdd:
      selftest_ld(f[0], in, 0);
      selftest_ld(f[1], in, 1);
      fe_add(o[0], f[0], f[1]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeSub:
      selftest_ld(f[0], in, 0);
      selftest_ld(f[1], in, 1);
      fe_sub(o[0], f[0], f[1]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeNeg:
      selftest_ld(f[0], in, 0);
      fe_neg(o[0], f[0]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeSubNc2:
      selftest_ld(f[0], in, 0);
      selftest_ld(f[1], in, 1);
      fe_sub_nc<2>(o[0], f[0], f[1]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeSubNc3:
      selftest_ld(f[0], in, 0);
      selftest_ld(f[1], in, 1);
      fe_sub_nc<3>(o[0], f[0], f[1]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeNegNc2:
      selftest_ld(f[0], in, 0);
      fe_neg_nc<2>(o[0], f[0]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeCarry:
      selftest_ld(o[0], in, 0);
      fe_carry(o[0]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeCmov:
      selftest_ld(f[0], in, 0);
      selftest_ld(f[1], in, 1);
      fe_cmov(o[0], f[0], f[1], in[18] != 0);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeFrombytes:
      fe_frombytes(o[0], in);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeTobytes:
      selftest_ld(f[0], in, 0);
      fe_tobytes(out, f[0]);
      break;
    case kOpFeIszero:
      selftest_ld(f[0], in, 0);
      flag[0] = fe_iszero(f[0]) ? 1u : 0u;
      break;
    case kOpFeIsnegative:
      selftest_ld(f[0], in, 0);
      flag[0] = fe_isnegative(f[0]);
      break;
    case kOpFeInvert:
      selftest_ld(f[0], in, 0);
      fe_invert(o[0], f[0]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFePow22523:
      selftest_ld(f[0], in, 0);
      fe_pow22523(o[0], f[0]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeConstD:
      fe_const_d(o[0]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeConst2d:
      fe_const_2d(o[0]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpFeConstSqrtm1:
      fe_const_sqrtm1(o[0]);
      selftest_st(out, 0, o[0]);
      break;
    case kOpScReduce64:
      sc_reduce64(out, in);
      break;
    case kOpScMuladd:
      sc_muladd(out, in, in + 8, in + 16);
      break;
    case kOpScLtL:
      flag[0] = sc_lt_L(in) ? 1u : 0u;
      break;
    case kOpScRecode16:
      sc_recode16(out, in);
      break;
    case kOpScRecode256:
      sc_recode256(out, in);
      break;
    case kOpScRecode65536:
      sc_recode65536(out, in);
      break;
    case kOpScMulSigned:
      sc_mul_signed(out, in, in[5] != 0, in + 8);
      break;
    case kOpLatticeHalf: {
      bool cn = false, dn = false;
      const bool ok = lattice_half(out, cn, out + 5, dn, in);
      flag[0] = ok ? 1u : 0u;
      flag[1] = cn ? 1u : 0u;
      flag[2] = dn ? 1u : 0u;
      break;
    }
    case kOpScRecode16Half:
      flag[0] = (uint32_t)sc_recode16_half(out, in);
      break;
    case kOpGeP2Dbl:
    case kOpGeP2DblLazy: {
      ge_p2 p;
      ge_p1p1 r;
      selftest_ld_p2(p, in);
      if (op == kOpGeP2DblLazy)
        ge_p2_dbl<true>(r, p);
      else
        ge_p2_dbl<false>(r, p);
      selftest_st_p1p1(out, r);
      break;
    }
    case kOpGeAffineDbl: {
      ge_p3 p;
      ge_p1p1 r;
      selftest_ld_p3(p, in);
      ge_affine_dbl(r, p);
      selftest_st_p1p1(out, r);
      break;
    }
    case kOpGeAddCached: {
      ge_p3 p;
      ge_cached c;
      ge_p1p1 r;
      selftest_ld_p3(p, in);
      selftest_ld_cached(c, in, 4);
      ge_add_cached(r, p, c);
      selftest_st_p1p1(out, r);
      break;
    }
    case kOpGeMadd: {
      ge_p3 p;
      ge_niels n;
      ge_p1p1 r;
      selftest_ld_p3(p, in);
      selftest_ld_niels(n, in, 4);
      ge_madd(r, p, n);
      selftest_st_p1p1(out, r);
      break;
    }
    case kOpGeP1p1ToP2: {
      ge_p1p1 t;
      ge_p2 r;
      selftest_ld_p1p1(t, in);
      ge_p1p1_to_p2(r, t);
      selftest_st(out, 0, r.X);
      selftest_st(out, 1, r.Y);
      selftest_st(out, 2, r.Z);
      break;
    }
    case kOpGeP1p1ToP3: {
      ge_p1p1 t;
      ge_p3 r;
      selftest_ld_p1p1(t, in);
      ge_p1p1_to_p3(r, t);
      selftest_st_p3(out, r);
      break;
    }
    case kOpGeP3ToCached: {
      ge_p3 p;
      ge_cached c;
      selftest_ld_p3(p, in);
      ge_p3_to_cached(c, p);
      selftest_st(out, 0, c.YpX);
      selftest_st(out, 1, c.YmX);
      selftest_st(out, 2, c.Z);
      selftest_st(out, 3, c.T2d);
      break;
    }
    case kOpGeCachedCneg: {
      ge_cached c;
      selftest_ld_cached(c, in, 0);
      ge_cached_cneg(c, in[36] != 0);
      selftest_st(out, 0, c.YpX);
      selftest_st(out, 1, c.YmX);
      selftest_st(out, 2, c.Z);
      selftest_st(out, 3, c.T2d);
      break;
    }
    case kOpGeNielsCneg: {
      ge_niels n;
      selftest_ld_niels(n, in, 0);
      ge_niels_cneg(n, in[27] != 0);
      selftest_st(out, 0, n.ypx);
      selftest_st(out, 1, n.ymx);
      selftest_st(out, 2, n.xy2d);
      break;
    }
    case kOpGeFrombytesNegate: {
      ge_p3 r;
      const bool ok = ge_frombytes_negate_vartime(r, in);
      selftest_st_p3(out, r);
      flag[0] = ok ? 1u : 0u;
      break;
    }
    case kOpGeTobytes: {
      ge_p2 p;
      selftest_ld_p2(p, in);
      ge_tobytes(out, p);
      break;
    }
    default:
      break;
  }
}

}  // namespace stl
