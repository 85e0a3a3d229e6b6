// stl_hash160.h -- Hash160 of a 32-byte account public key, for the gfx950
// kernels and their host build.
//
// Reference path:
//   RippleAddress::getAccountID() = Hash160(vchData)       RippleAddress.cpp:361-363
//   Hash160(x) = RIPEMD160(SHA256(x))                       HashUtilities.cpp:22-29
// An ed25519 account public key is 32 bytes, and so is the SHA-256 digest
// RIPEMD-160 then hashes: both hashes see exactly one block whose padding is
// known at compile time.  Only that size is implemented.  Everything is
// written so that it stays in registers on the device: the message words are
// separate values after unrolling (every index a constant), the rotations are
// by constants, and no table is indexed by a run-time value.
//
// Byte order: every "le words" array holds the bytes of the message or digest
// in memory order, as little-endian 32-bit words (what a dword load of the
// bytes gives on gfx950 and on the host).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef STL_HD
#define STL_HD __host__ __device__ __forceinline__
#endif

namespace stl {

STL_HD uint32_t h160_rol(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
STL_HD uint32_t h160_ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
STL_HD uint32_t h160_bswap(uint32_t x) { return __builtin_bswap32(x); }

// ---- SHA-256 (FIPS 180-4) of 32 bytes ----
STL_HD uint32_t sha256_k(int i) {
  // indexed with a compile-time i after unrolling
  const uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  return K[i];
}

// out = SHA-256(m), m 32 bytes: one block, words 8..15 are the padding
// (0x80, zeros, the bit length 256).
STL_HD void sha256_32(const uint32_t m_le[8], uint32_t out_le[8]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = h160_bswap(m_le[i]);
  w[8] = 0x80000000u;
#pragma unroll
  for (int i = 9; i < 15; ++i) w[i] = 0u;
  w[15] = 256u;
  const uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                          0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint32_t a = iv[0], b = iv[1], c = iv[2], d = iv[3], e = iv[4], f = iv[5], g = iv[6], h = iv[7];
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    if (i >= 16) {
      const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      const uint32_t s0 = h160_ror(w15, 7) ^ h160_ror(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = h160_ror(w2, 17) ^ h160_ror(w2, 19) ^ (w2 >> 10);
      w[i & 15] = w[i & 15] + s0 + w[(i + 9) & 15] + s1;
    }
    const uint32_t S1 = h160_ror(e, 6) ^ h160_ror(e, 11) ^ h160_ror(e, 25);
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = h + S1 + ch + sha256_k(i) + w[i & 15];
    const uint32_t S0 = h160_ror(a, 2) ^ h160_ror(a, 13) ^ h160_ror(a, 22);
    const uint32_t maj = (a & b) ^ (a & c) ^ (b & c);
    const uint32_t t2 = S0 + maj;
    h = g; g = f; f = e; e = d + t1;
    d = c; c = b; b = a; a = t1 + t2;
  }
  out_le[0] = h160_bswap(a + iv[0]);
  out_le[1] = h160_bswap(b + iv[1]);
  out_le[2] = h160_bswap(c + iv[2]);
  out_le[3] = h160_bswap(d + iv[3]);
  out_le[4] = h160_bswap(e + iv[4]);
  out_le[5] = h160_bswap(f + iv[5]);
  out_le[6] = h160_bswap(g + iv[6]);
  out_le[7] = h160_bswap(h + iv[7]);
}

// ---- RIPEMD-160 (Dobbertin, Bosselaers, Preneel 1996) of 32 bytes ----
// Message word and rotation of step j (0..79) of the left and the right line.
STL_HD int rmd_rl(int j) {
  const int8_t r[80] = {0, 1, 2,  3,  4,  5,  6,  7, 8,  9, 10, 11, 12, 13, 14, 15,
                        7, 4, 13, 1,  10, 6,  15, 3, 12, 0, 9,  5,  2,  14, 11, 8,
                        3, 10, 14, 4, 9,  15, 8,  1, 2,  7, 0,  6,  13, 11, 5,  12,
                        1, 9, 11, 10, 0,  8,  12, 4, 13, 3, 7,  15, 14, 5,  6,  2,
                        4, 0, 5,  9,  7,  12, 2,  10, 14, 1, 3, 8,  11, 6,  15, 13};
  return r[j];
}
STL_HD int rmd_rr(int j) {
  const int8_t r[80] = {5,  14, 7,  0, 9, 2,  11, 4,  13, 6,  15, 8,  1,  10, 3,  12,
                        6,  11, 3,  7, 0, 13, 5,  10, 14, 15, 8,  12, 4,  9,  1,  2,
                        15, 5,  1,  3, 7, 14, 6,  9,  11, 8,  12, 2,  10, 0,  4,  13,
                        8,  6,  4,  1, 3, 11, 15, 0,  5,  12, 2,  13, 9,  7,  10, 14,
                        12, 15, 10, 4, 1, 5,  8,  7,  6,  2,  13, 14, 0,  3,  9,  11};
  return r[j];
}
STL_HD int rmd_sl(int j) {
  const int8_t s[80] = {11, 14, 15, 12, 5,  8,  7,  9,  11, 13, 14, 15, 6,  7,  9,  8,
                        7,  6,  8,  13, 11, 9,  7,  15, 7,  12, 15, 9,  11, 7,  13, 12,
                        11, 13, 6,  7,  14, 9,  13, 15, 14, 8,  13, 6,  5,  12, 7,  5,
                        11, 12, 14, 15, 14, 15, 9,  8,  9,  14, 5,  6,  8,  6,  5,  12,
                        9,  15, 5,  11, 6,  8,  13, 12, 5,  12, 13, 14, 11, 8,  5,  6};
  return s[j];
}
STL_HD int rmd_sr(int j) {
  const int8_t s[80] = {8,  9,  9,  11, 13, 15, 15, 5,  7,  7,  8,  11, 14, 14, 12, 6,
                        9,  13, 15, 7,  12, 8,  9,  11, 7,  7,  12, 7,  6,  15, 13, 11,
                        9,  7,  15, 11, 8,  6,  6,  14, 12, 13, 5,  14, 13, 13, 7,  5,
                        15, 5,  8,  11, 14, 14, 6,  14, 6,  9,  12, 9,  12, 5,  15, 8,
                        8,  5,  12, 9,  12, 5,  14, 6,  8,  13, 6,  5,  15, 13, 11, 11};
  return s[j];
}

// The five round functions; the left line uses F in round F, the right line
// 4 - F.
template <int F>
STL_HD uint32_t rmd_f(uint32_t x, uint32_t y, uint32_t z) {
  static_assert(F >= 0 && F < 5, "round");
  if (F == 0) return x ^ y ^ z;
  if (F == 1) return (x & y) | (~x & z);
  if (F == 2) return (x | ~y) ^ z;
  if (F == 3) return (x & z) | (y & ~z);
  return x ^ (y | ~z);
}

// Round R (16 steps) of both lines.  l and r hold {A, B, C, D, E}.
template <int R>
STL_HD void rmd_round(uint32_t l[5], uint32_t r[5], const uint32_t x[16]) {
  const uint32_t kl[5] = {0x00000000u, 0x5a827999u, 0x6ed9eba1u, 0x8f1bbcdcu, 0xa953fd4eu};
  const uint32_t kr[5] = {0x50a28be6u, 0x5c4dd124u, 0x6d703ef3u, 0x7a6d76e9u, 0x00000000u};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int j = 16 * R + i;
    uint32_t t = h160_rol(l[0] + rmd_f<R>(l[1], l[2], l[3]) + x[rmd_rl(j)] + kl[R], rmd_sl(j)) + l[4];
    l[0] = l[4]; l[4] = l[3]; l[3] = h160_rol(l[2], 10); l[2] = l[1]; l[1] = t;
    t = h160_rol(r[0] + rmd_f<4 - R>(r[1], r[2], r[3]) + x[rmd_rr(j)] + kr[R], rmd_sr(j)) + r[4];
    r[0] = r[4]; r[4] = r[3]; r[3] = h160_rol(r[2], 10); r[2] = r[1]; r[1] = t;
  }
}

// out = RIPEMD-160(m), m 32 bytes: one block, words 8..15 are the padding
// (0x80, zeros, the bit length 256 in word 14).
STL_HD void ripemd160_32(const uint32_t m_le[8], uint32_t out_le[5]) {
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = m_le[i];
  x[8] = 0x00000080u;
#pragma unroll
  for (int i = 9; i < 16; ++i) x[i] = 0u;
  x[14] = 256u;
  const uint32_t iv[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
  uint32_t l[5], r[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) l[i] = r[i] = iv[i];
  rmd_round<0>(l, r, x);
  rmd_round<1>(l, r, x);
  rmd_round<2>(l, r, x);
  rmd_round<3>(l, r, x);
  rmd_round<4>(l, r, x);
  out_le[0] = iv[1] + l[2] + r[3];
  out_le[1] = iv[2] + l[3] + r[4];
  out_le[2] = iv[3] + l[4] + r[0];
  out_le[3] = iv[4] + l[0] + r[1];
  out_le[4] = iv[0] + l[1] + r[2];
}

// Hash160 of a 32-byte public key: the 20 bytes RippleAddress::getAccountID
// returns, in OpenSSL's byte order, as five little-endian words.
STL_HD void hash160_32(const uint32_t pk_le_words[8], uint32_t out_le_words[5]) {
  uint32_t d[8];
  sha256_32(pk_le_words, d);
  ripemd160_32(d, out_le_words);
}

}  // namespace stl
