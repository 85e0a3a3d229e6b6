// stl_comb.h -- doubling-free verification for registered signers (the
// keyset, include/stl.h): per-key fixed-window ("comb") tables of
// j * 2^(8w) * (-A), and one of j * 2^(8w) * B, so that
//     R' = [S]B + [k](-A)
// is 64 mixed additions of table rows and no doubling.  encode(R') == R is
// then libsodium's predicate literally: R is never decoded, and the table is
// built on the actual decoded point, so mixed-order and small-order keys give
// the same group element as the Straus loop of stl_verify_core.h.
//
// Same code for the host (tests/native/hostemu_keyset.cpp) and the device
// (stl_keyset.hip).  Limb bounds are annotated as [alpha] (stl_fe25519.h).
#pragma once
#include "stl_verify_core.h"

namespace stl {

// ---- geometry ----
// Signed radix-256 digits (sc_recode256: digits 0..30 in [-128, 127], digit
// 31 in [0, 32]), one window per digit, rows |j| = 1..128 per window, one
// aligned 128-B line per row: 27 Niels limbs + 5 zero pad words.
constexpr int kCombBits = 8;
constexpr int kCombWindows = 32;
constexpr int kCombRows = 128;
constexpr int kCombRowWords = 32;
constexpr int kCombRowQuads = 7;  // the quads of a row that hold limbs (27 of 28 words)
constexpr size_t kCombKeyWords = (size_t)kCombWindows * kCombRows * kCombRowWords;  // 512 KiB per key
// Montgomery's trick over one window's 128 rows: the running products of Z
constexpr size_t kCombScratchWords = (size_t)kCombRows * 9;  // per (key, window) lane

// ---- per-key record (32 words), written once at registration ----
//   words 0-7   the key's 32 bytes (hashed into k)
//   words 8-16  x of the decoded point the table is built on (-A; +B for the base), [1]
//   words 17-25 y
//   word 26     flags below
constexpr int kKeyRecWords = 32;
constexpr int kKeyRecX = 8, kKeyRecY = 17, kKeyRecFlags = 26;
enum : uint32_t {
  kKeyDecodes = 1u,     // ge_frombytes_negate_vartime succeeded: the key has rows
  kKeyCanonical = 2u,   // point_is_canonical
  kKeySmallOrder = 4u,  // has_small_order
  kKeyAllZero = 8u,     // all_zero
};

// Decodes key bytes A into its record.  plus: store +A instead of -A (the
// base point's table is built from B's encoding).
STL_HD void comb_key_record(uint32_t rec[kKeyRecWords], const uint32_t A[8], bool plus) {
  ge_p3 P;
  const bool ok = ge_frombytes_negate_vartime(P, A);  // X, Y [1]
  fe nx;
  fe_neg(nx, P.X);                                     // [1]
  fe_cmov(P.X, P.X, nx, plus);
#pragma unroll
  for (int i = 0; i < 8; ++i) rec[i] = A[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    rec[kKeyRecX + i] = P.X.v[i];
    rec[kKeyRecY + i] = P.Y.v[i];
  }
  rec[kKeyRecFlags] = (ok ? kKeyDecodes : 0u) | (point_is_canonical(A) ? kKeyCanonical : 0u) |
                      (has_small_order(A) ? kKeySmallOrder : 0u) | (all_zero(A) ? kKeyAllZero : 0u);
#pragma unroll
  for (int i = kKeyRecFlags + 1; i < kKeyRecWords; ++i) rec[i] = 0;
}

STL_HD void comb_record_point(ge_p3& P, const uint32_t rec[kKeyRecWords]) {
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    P.X.v[i] = rec[kKeyRecX + i];
    P.Y.v[i] = rec[kKeyRecY + i];
  }
  fe_1(P.Z);
  fe_mul(P.T, P.X, P.Y);  // 1 * 1
}

// W = 2^(8w) * P for an affine P: 8w doublings (p3 [1] throughout:
// ge_p2_dbl takes [1], ge_p1p1_to_p3 gives [1 + 2^-12]).
STL_HD void comb_window_base(ge_p3& W, const ge_p3& P, int w) {
  W = P;
#pragma unroll 1
  for (int i = 0; i < kCombBits * w; ++i) {
    ge_p2 q;
    ge_p1p1 t;
    ge_p3_to_p2(q, W);
    ge_p2_dbl(t, q);
    ge_p1p1_to_p3(W, t);
  }
}

// The canonical representative (limbs < 2^29, value < p) of f [<= 3].
STL_HD void fe_canonical(fe& h, const fe& f) {
  uint32_t w[8];
  fe_tobytes(w, f);
  fe_frombytes(h, w);
}

// One window of one key: rows[(j-1) * kCombRowWords ...] = Niels form
// (y+x, y-x, 2dxy) of j * W, j = 1..128, every limb canonical, pad words 0.
// Pass 1 adds W 127 times (add-2008-hwcd-3 is complete on this curve, so
// torsion points, doublings and the identity need no special case, and Z is
// never 0), parks X, Y, Z in the row itself and the running product of Z in
// `scratch`; pass 2 walks back with one inversion for all 128 rows.
STL_HD void comb_build_window(uint32_t* rows, uint32_t* scratch, const ge_p3& W) {
  ge_cached Wc;
  ge_p3_to_cached(Wc, W);  // [1; T2d 1]
  ge_p3 P = W;
  fe c;
  fe_1(c);
#pragma unroll 1
  for (int j = 1; j <= kCombRows; ++j) {
    uint32_t* row = rows + (size_t)(j - 1) * kCombRowWords;
    fe_mul(c, c, P.Z);  // 1 * 1
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      row[i] = P.X.v[i];
      row[9 + i] = P.Y.v[i];
      row[18 + i] = P.Z.v[i];
      scratch[(size_t)(j - 1) * 9 + i] = c.v[i];
    }
    if (j < kCombRows) {
      ge_p1p1 t;
      ge_add_cached(t, P, Wc);  // p3 [1] + cached [1]
      ge_p1p1_to_p3(P, t);
    }
  }
  fe inv, c2d;
  fe_invert(inv, c);  // 1 / (Z_1 ... Z_128)
  fe_const_2d(c2d);
#pragma unroll 1
  for (int j = kCombRows; j >= 1; --j) {
    uint32_t* row = rows + (size_t)(j - 1) * kCombRowWords;
    fe X, Y, Z, prev, zi, x, y, xy, t;
    fe_1(prev);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      X.v[i] = row[i];
      Y.v[i] = row[9 + i];
      Z.v[i] = row[18 + i];
      if (j > 1) prev.v[i] = scratch[(size_t)(j - 2) * 9 + i];
    }
    fe_mul2(zi, inv, prev, inv, inv, Z);  // 1 / Z_j; inv = 1 / (Z_1 ... Z_{j-1})   (1 * 1)
    fe_mul2(x, X, zi, y, Y, zi);
    fe_mul(xy, x, y);
    fe_mul(xy, xy, c2d);
    fe_add(t, y, x);                      // [2]
    fe_carry(t);                          // [1]
    fe_canonical(t, t);
#pragma unroll
    for (int i = 0; i < 9; ++i) row[i] = t.v[i];
    fe_sub(t, y, x);                      // [1]
    fe_canonical(t, t);
#pragma unroll
    for (int i = 0; i < 9; ++i) row[9 + i] = t.v[i];
    fe_canonical(t, xy);
#pragma unroll
    for (int i = 0; i < 9; ++i) row[18 + i] = t.v[i];
#pragma unroll
    for (int i = 27; i < kCombRowWords; ++i) row[i] = 0;
  }
}

// ---- lookups ----
// A row in flight: the 7 quads that hold its 27 limbs.
struct CombRow {
  uint4 q[kCombRowQuads];
};

// Requests row (w, |digit|) of `table` (one key's kCombKeyWords); digit 0
// requests row 1 of the window (replaced by the identity in comb_row_niels).
// live = false reads nothing (a lane with no key).
STL_HD void comb_row_load(CombRow& r, const uint32_t* table, int w, int digit, bool live) {
  const int a = digit < 0 ? -digit : digit;
  const int j = a > kCombRows ? kCombRows : (a > 0 ? a : 1);
#pragma unroll
  for (int i = 0; i < kCombRowQuads; ++i) r.q[i] = make_uint4(0u, 0u, 0u, 0u);
  if (live) {
    const uint4* p = reinterpret_cast<const uint4*>(table + ((size_t)w * kCombRows + (size_t)(j - 1)) * kCombRowWords);
#pragma unroll
    for (int i = 0; i < kCombRowQuads; ++i) r.q[i] = p[i];
  }
}

// sign(digit) * row, or the identity Niels (1, 1, 0) for digit 0 (as
// load_base_niels): [1; xy2d <= 2].
STL_HD void comb_row_niels(ge_niels& n, const CombRow& r, int digit) {
  uint32_t w[4 * kCombRowQuads];
#pragma unroll
  for (int i = 0; i < kCombRowQuads; ++i) {
    w[4 * i] = r.q[i].x;
    w[4 * i + 1] = r.q[i].y;
    w[4 * i + 2] = r.q[i].z;
    w[4 * i + 3] = r.q[i].w;
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    n.ypx.v[i] = w[i];
    n.ymx.v[i] = w[9 + i];
    n.xy2d.v[i] = w[18 + i];
  }
  ge_niels id;
  fe_1(id.ypx);
  fe_1(id.ymx);
  fe_0(id.xy2d);
  const bool z = digit == 0;
  fe_cmov(n.ypx, n.ypx, id.ypx, z);
  fe_cmov(n.ymx, n.ymx, id.ymx, z);
  fe_cmov(n.xy2d, n.xy2d, id.xy2d, z);
  ge_niels_cneg(n, digit < 0);
}

// out = [k]P + [S]B from the tables of P (`key`, built on -A) and of B
// (`base`): kd / sd are sc_recode256 digits.  64 ge_madd, no doubling.  The
// digit string is known up front, so each row is requested one window (two
// additions) before it is used: while window w's two additions run, window
// w+1's two lines are in flight.  Digits are taken from the low end of kd / sd
// by shifting the arrays (no dynamic register index).
STL_HD void comb_double_scalarmult(ge_p2& out, const uint32_t kd_in[8], const uint32_t sd_in[8], const uint32_t* key,
                                   const uint32_t* base, bool live) {
  uint32_t kd[8], sd[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    kd[i] = kd_in[i];
    sd[i] = sd_in[i];
  }
  uint32_t wk = kd[0], ws = sd[0];
  int dk = (int32_t)(wk << 24) >> 24, ds = (int32_t)(ws << 24) >> 24;
  CombRow rk, rs;
  comb_row_load(rk, key, 0, dk, live);
  comb_row_load(rs, base, 0, ds, live);
  ge_p3 acc;
  ge_p3_0(acc);
  ge_p1p1 t;
#pragma unroll 1
  for (int w = 0; w < kCombWindows; ++w) {
    // the next window's digits
    if ((w & 3) == 3) {
#pragma unroll
      for (int m = 0; m < 7; ++m) {
        kd[m] = kd[m + 1];
        sd[m] = sd[m + 1];
      }
      wk = kd[0];
      ws = sd[0];
    } else {
      wk >>= 8;
      ws >>= 8;
    }
    const int dk1 = (int32_t)(wk << 24) >> 24, ds1 = (int32_t)(ws << 24) >> 24;
    const bool more = w + 1 < kCombWindows;
    ge_niels n;
    comb_row_niels(n, rk, dk);
    if (more) comb_row_load(rk, key, w + 1, dk1, live);
    ge_madd(t, acc, n);      // p3 [1] + niels [1; 2]
    ge_p1p1_to_p3(acc, t);
    comb_row_niels(n, rs, ds);
    if (more) comb_row_load(rs, base, w + 1, ds1, live);
    ge_madd(t, acc, n);
    if (more) ge_p1p1_to_p3(acc, t);
    dk = dk1;
    ds = ds1;
  }
  ge_p1p1_to_p2(out, t);
}

// The encoding of [S]B + [k](-A) by the comb (S masked to 253 bits as
// verify_phase2 masks it; k < L).
STL_HD void comb_point_bytes(uint32_t enc[8], const uint32_t k[8], const uint32_t S[8], const uint32_t* key,
                             const uint32_t* base, bool live) {
  uint32_t Sm[8], kd[8], sd[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) Sm[i] = S[i];
  Sm[7] &= 0x1fffffffu;
  sc_recode256(kd, k);
  sc_recode256(sd, Sm);
  ge_p2 Rp;
  comb_double_scalarmult(Rp, kd, sd, key, base, live);
  ge_tobytes(enc, Rp);
}

// The accept predicate for a registered key: verify_prechecks and
// composite_s_ok with the key's share read from its flags, then
// encode([S]B + [k](-A)) == R.  policy: kPolicy* (bit 0, kPolicyRaw).
STL_HD bool verify_comb_with_k(const uint32_t R[8], const uint32_t S[8], uint32_t kflags, const uint32_t k[8],
                               uint32_t policy, const uint32_t* key, const uint32_t* base) {
  bool ok;
  if ((policy & 1u) == kPolicyStellard100)
    ok = (S[7] >> 29) == 0 && !(kflags & kKeyAllZero);  // sig[63] & 224
  else
    ok = sc_lt_L(S) && !has_small_order(R) && (kflags & kKeyCanonical) != 0 && !(kflags & kKeySmallOrder);
  ok = ok && (kflags & kKeyDecodes) != 0 && composite_s_ok(S, policy);
  uint32_t enc[8];
  comb_point_bytes(enc, k, S, key, base, (kflags & kKeyDecodes) != 0);
  bool eq = true;
#pragma unroll
  for (int i = 0; i < 8; ++i) eq = eq && enc[i] == R[i];
  return ok && eq;
}

}  // namespace stl
