// stl_keycache.h -- the per-device cache of decoded public keys.
//
// Decoding a key A (ge_frombytes_negate_vartime) is a square root: one
// fe_pow22523 chain, about 21 k lane instructions, and a pure function of the
// key's 32 bytes.  stellard's signers sign again in every ledger, so the cache
// keeps x(-A) from one call to the next and a row whose key is found there
// skips the chain.
//
// NOTHING READ FROM THE CACHE IS TRUSTED.  A slot offers a candidate x for a
// key; key_cache_certify checks it against the row's own key bytes before it
// is used, with about five field products.  Let y = fe_frombytes(A),
// u = y^2 - 1, v = d y^2 + 1 and X the candidate.  The candidate passes iff
//     v X^2 - u == 0,   X != 0,   fe_isnegative(X) != (A[7] >> 31).
// Why a pass means "the decoder returns ok with exactly this X (mod p)":
//   * v is never zero: v == 0 needs y^2 == -1/d, and -1/d is a non-square
//     (d is a non-square, -1 a square, p == 1 mod 4);
//   * so v X^2 == u says u/v is the square X^2.  Then the decoder's candidate
//     x = u v^3 (u v^7)^((p-5)/8) has v x^2 == u or v x^2 == -u, it takes x or
//     x sqrt(-1) accordingly and returns ok, and its x is one of the two roots
//     +-X of u/v;
//   * X != 0 makes the two roots differ in parity, and the decoder's last step
//     leaves the one with fe_isnegative(x) != sign bit on -A: the third
//     condition picks the same one.
// The y the row uses is always taken from its own key bytes.  So a stale, torn,
// evicted, concurrently overwritten or poisoned slot can only fail the check
// (the row then takes the chain, as without a cache): it can cost speed, never
// an accept bit.  That is why the cache needs no locks, state words, fences or
// quiescent clear; how soon one workgroup's insert is seen by another only
// moves the hit rate.
//
// Keys whose decoding fails, and keys with x == 0 (y == +-1), are never
// cached and never hit.
//
// Geometry: 2^K sets (K = kKeyCacheLog2Default; STL_KEY_CACHE_LOG2) of 256 B,
// each with kKeyCacheWays = 6 slots.  A slot is a 64-bit tag of the key and
// the canonical 32 bytes (fe_tobytes) of x(-A).  Inside a set the tags come
// first, so that a lookup reads 48 B of tags and then one x:
//     words  0..11   tag of way 0..5 (2 words each)
//     words 12..15   zero
//     words 16..63   x of way 0..5 (8 words each)
// The key itself is not stored: a wrong x fails the check whatever key it
// belonged to, so a tag that matches the wrong key only costs a miss.  With
// 2^20 keys in 2^20 sets (Poisson, mean 1) 1.9 % of the keys lie in a set that
// holds more than 4 of them, 0.06 % in one that holds more than 6 -- hence six
// tagged 40-B slots rather than four 64-B slots with the key's bytes, in the
// same 256 B.  An empty slot is all zero (tag and x; its x never certifies).
// The set index is key_hash & (2^K - 1); the way an insert starts from comes
// from the hash's top byte, which no mask up to 2^24 uses.
//
// Those 0.06 % (about 600 of 2^20 keys) would miss on every call.  So a key has
// a second-choice set (key_cache_alt_set, from the key alone, never its
// primary set): an insert goes there only when the primary set holds neither
// the key's tag nor an empty way (key_cache_place), and a lookup reads the
// alternate set's tags only when the primary set's hold no match -- a warm
// lookup still gathers one set for all but those keys.  What either set offers
// goes through the same check.
//
// Plain C++ for the host and the device (tests/native/hostemu_keycache.cpp).
#pragma once
#include "stl_fe25519.h"

namespace stl {

constexpr int kKeyCacheLog2Default = 20;
constexpr int kKeyCacheLog2Min = 10, kKeyCacheLog2Max = 24;
constexpr uint32_t kKeyCacheWays = 6;
constexpr uint32_t kKeyCacheSetBytes = 256;      // all a row gathers, at most
constexpr uint32_t kKeyCacheTagWord = 0;         // word of way w's tag: kKeyCacheTagWord + 2 w
constexpr uint32_t kKeyCacheXWord = 16;          // word of way w's x: kKeyCacheXWord + 8 w
static_assert(2 * kKeyCacheWays <= kKeyCacheXWord && (kKeyCacheXWord + 8 * kKeyCacheWays) * 4 == kKeyCacheSetBytes,
              "tags, then the xs, fill the set");
inline size_t key_cache_bytes(int log2_sets) { return (size_t)kKeyCacheSetBytes << log2_sets; }

// 32-bit hash of a key's bytes: the per-batch key dedup's table index and the
// cache's set index (its low bits) and first way (its top bits).
STL_HD uint32_t key_hash(const uint32_t A[8]) {
  uint32_t h = A[0] * 0x9E3779B1u;
  h ^= A[1] * 0x85EBCA6Bu;
  h = (h << 13) | (h >> 19);
  h ^= A[2] * 0xC2B2AE35u;
  h ^= A[5] * 0x27D4EB2Fu;
  h ^= h >> 16;
  return h * 0x7FEB352Du;
}

STL_HD uint32_t key_cache_set(uint32_t hash, uint32_t mask) { return hash & mask; }
STL_HD uint32_t key_cache_first_way(uint32_t hash) { return ((hash >> 24) * kKeyCacheWays) >> 8; }
static_assert(kKeyCacheLog2Max <= 24, "the way bits lie above every set mask");
// The key's second-choice set.  key_hash's 32 bits are all spoken for at the
// largest mask (24 of set index, 8 of first way), so the offset from the
// primary set comes from a second word of hash over the key, mixed from the
// four words key_hash leaves out or weighs least: a function of the key alone
// and independent of the primary index.  The offset is forced non-zero inside
// the mask (its lowest bit, where the hash's bits there are all zero), so the
// two sets differ whenever the mask has a bit, i.e. more than one set is in
// use; with mask 0 both are set 0.
STL_HD uint32_t key_cache_alt_set(const uint32_t A[8], uint32_t mask) {
  uint32_t g = A[3] * 0xC2B2AE35u;
  g ^= A[6] * 0x27D4EB2Fu;
  g = (g << 15) | (g >> 17);
  g ^= A[4] * 0x9E3779B1u;
  g ^= A[7] * 0x85EBCA6Bu;
  g ^= g >> 15;
  g *= 0x2C1B3C6Du;
  g ^= g >> 13;
  uint32_t off = g & mask;
  if (off == 0) off = mask & (0u - mask);
  return key_cache_set(key_hash(A), mask) ^ off;
}
// The key's tag, from the words key_hash leaves out and the two it weighs
// least: independent of the set index.
STL_HD void key_cache_tag(uint32_t tag[2], const uint32_t A[8]) {
  tag[0] = A[3] ^ (A[6] * 0x9E3779B1u) ^ (A[0] >> 7);
  tag[1] = A[4] ^ (A[7] * 0x85EBCA6Bu) ^ (A[1] << 9);
}

// The slot an insert of a key overwrites, given for each way of its set
// whether it holds this key's tag (same: a stale or bad x is replaced where
// lookups will find it -- a lookup takes the lowest way with the key's tag,
// and so does this) and whether it is all zero (empty).  Otherwise the
// first empty way counting from the hash's way, otherwise the hash's way.
// Starting at the hash's way, not at way 0, lets keys that meet in one set
// during one call mostly land in different ways at once.
STL_HD uint32_t key_cache_victim(uint32_t hash, const bool same[kKeyCacheWays], const bool empty[kKeyCacheWays]) {
  const uint32_t first = key_cache_first_way(hash);
  uint32_t v = first;
#pragma unroll
  for (int i = (int)kKeyCacheWays - 1; i >= 0; --i) {  // the nearest empty way is assigned last
    const uint32_t w = (first + (uint32_t)i) % kKeyCacheWays;
    if (empty[w]) v = w;
  }
#pragma unroll
  for (int w = (int)kKeyCacheWays - 1; w >= 0; --w)  // the lowest such way: the one a lookup tries
    if (same[w]) v = (uint32_t)w;
  return v;
}

// Where an insert writes, over the key's two sets (bit w of same0 / empty0:
// way w of the primary set holds the key's tag / is all zero; same1 / empty1
// likewise for the alternate set, which a caller need only read when the
// primary set offers nothing and may pass as 0, 0 otherwise).  An insert
// writes where the next lookup looks first:
//   1. the way holding the key's tag in the primary set,
//   2. an empty primary way (key_cache_victim),
//   3. the way holding the key's tag in the alternate set,
//   4. an empty alternate way (key_cache_victim in that set),
//   5. the primary set's hash way.
// Returns the way; `alt` says which set.
STL_HD uint32_t key_cache_place(uint32_t hash, uint32_t same0, uint32_t empty0, uint32_t same1, uint32_t empty1,
                                bool& alt) {
  alt = (same0 | empty0) == 0u && (same1 | empty1) != 0u;
  const uint32_t sb = alt ? same1 : same0, eb = alt ? empty1 : empty0;
  bool same[kKeyCacheWays], empty[kKeyCacheWays];
#pragma unroll
  for (uint32_t w = 0; w < kKeyCacheWays; ++w) {
    same[w] = ((sb >> w) & 1u) != 0;
    empty[w] = ((eb >> w) & 1u) != 0;
  }
  return key_cache_victim(hash, same, empty);
}

// Branch-free.  X = fe_frombytes(xbytes); true iff X is the x of -A as
// ge_frombytes_negate_vartime returns it (mod p), non-zero -- see the top.
STL_HD bool key_cache_certify(fe& X, const uint32_t A[8], const uint32_t xbytes[8]) {
  fe y, u, v, one, d, xx, chk;
  fe_frombytes(y, A);
  fe_frombytes(X, xbytes);
  fe_1(one);
  fe_const_d(d);
  fe_sq2(u, y, xx, X);       // y^2, X^2
  fe_mul(v, u, d);
  fe_sub(u, u, one);         // u = y^2 - 1
  fe_add(v, v, one);         // v = d y^2 + 1   [2]
  fe_mul(xx, xx, v);         // v X^2           (1 * 2 <= 7)
  fe_sub(chk, xx, u);
  uint32_t cw[8], xw[8];
  fe_tobytes(cw, chk);
  fe_tobytes(xw, X);
  uint32_t cz = 0, xz = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    cz |= cw[i];
    xz |= xw[i];
  }
  const uint32_t sign = A[7] >> 31;
  return (cz == 0) & (xz != 0) & ((xw[0] & 1u) != sign);
}

}  // namespace stl
