// stl_shamap_core.h -- the SHAMap root of a set of 32-byte keys: what the
// device kernels (stl_shamap.hip) and the host emulation
// (tests/native/hostemu_shamap.cpp) share.
//
// The tree (SHAMap.cpp, SHAMapNodeID.cpp, SHAMapTreeNode.cpp of the node this
// library serves): an inner node has 16 branches; at depth d the branch of a
// key is its nibble d (byte d / 2, the high nibble for even d), so key order is
// memcmp order.  A leaf sits at the shallowest depth where its nibble prefix is
// unique, but never above depth 1; the root (depth 0) is always an inner node.
// An inner node's hash is SHA512Half("MIN\0" || h[0] .. h[15]), 516 bytes, with
// 32 zero bytes for an empty branch.
//
// Over the distinct keys k_0 < .. < k_{m-1}, with l_i the number of leading
// nibbles k_i and k_{i+1} share (l_{-1} = l_{m-1} = -1; for m = 1, l_0 counts
// as 0 so that the root exists): key i is the first key of an inner node at
// depth d exactly when l_{i-1} < d <= l_i.
#pragma once
#include "stl_sha512.h"

namespace stl {

constexpr uint32_t kShamapKeyWords = 8;      // a key, a hash: 8 little-endian dwords in memory order
constexpr uint32_t kShamapBranches = 16;
constexpr uint32_t kShamapDepths = 64;       // inner nodes live at depths 0 .. 63
constexpr uint32_t kShamapRecordWords = 129; // "MIN\0" and 16 slots: the preimage of an inner node's hash
constexpr uint32_t kShamapInnerPrefix = 0x004E494Du;  // the bytes 'M' 'I' 'N' 0 as a little-endian dword

// Nibble d (0 .. 63) of a key held as 8 memory-order dwords.
STL_HD uint32_t shamap_nibble(const uint32_t key[kShamapKeyWords], uint32_t d) {
  const uint32_t byte = (key[d >> 3] >> (8u * ((d >> 1) & 3u))) & 0xffu;
  return (d & 1u) ? (byte & 15u) : (byte >> 4);
}

// The same from bytes.
STL_HD uint32_t shamap_nibble_bytes(const uint8_t* key, uint32_t d) {
  const uint32_t byte = key[d >> 1];
  return (d & 1u) ? (byte & 15u) : (byte >> 4);
}

STL_HD uint32_t shamap_clz32(uint32_t x) {  // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__clz((int)x);
#else
  return (uint32_t)__builtin_clz(x);
#endif
}

// Leading nibbles two keys share: 0 .. 64 (64: equal).
STL_HD uint32_t shamap_common_prefix(const uint32_t a[kShamapKeyWords], const uint32_t b[kShamapKeyWords]) {
  for (uint32_t i = 0; i < kShamapKeyWords; ++i) {
    const uint32_t x = a[i] ^ b[i];
    if (x) return 8u * i + (shamap_clz32(bswap32(x)) >> 2);
  }
  return 64u;
}

// memcmp order of two keys: a < b.
STL_HD bool shamap_key_less(const uint32_t a[kShamapKeyWords], const uint32_t b[kShamapKeyWords]) {
  for (uint32_t i = 0; i < kShamapKeyWords; ++i) {
    if (a[i] != b[i]) return bswap32(a[i]) < bswap32(b[i]);
  }
  return false;
}

// The 64-bit sort word w (0: most significant) of a key, big-endian.
STL_HD uint64_t shamap_sort_word(const uint32_t key[kShamapKeyWords], uint32_t w) {
  return be64_from_le32(key[2 * w], key[2 * w + 1]);
}

// The neighbour byte of distinct key i: l_i as a signed byte, -1 .. 63.  `last`:
// key i is the greatest; `only`: it is also the least (m = 1).
STL_HD int32_t shamap_neighbour(const uint32_t key[kShamapKeyWords], const uint32_t next[kShamapKeyWords], bool last,
                                bool only) {
  if (only) return 0;
  if (last) return -1;
  return (int32_t)shamap_common_prefix(key, next);
}

// The node rule: a key whose neighbour bytes are l_prev (of the key before it;
// -1 for the first) and l_cur is the first key of an inner node at depth d.
STL_HD bool shamap_starts_node(int32_t l_prev, int32_t l_cur, int32_t d) { return l_prev < d && d <= l_cur; }

// The depth of the inner node a key's leaf hangs under.
STL_HD int32_t shamap_leaf_parent_depth(int32_t l_prev, int32_t l_cur) {
  const int32_t m = l_prev > l_cur ? l_prev : l_cur;
  return m > 0 ? m : 0;
}

STL_HD void shamap_load_key(uint32_t k[kShamapKeyWords], const uint8_t* keys, size_t pos) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = reinterpret_cast<const uint4*>(keys + 32 * pos);
  const uint4 a = q[0], b = q[1];
  k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w;
  k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
#else
  for (uint32_t i = 0; i < kShamapKeyWords; ++i) {
    const uint8_t* p = keys + 32 * pos + 4 * i;
    k[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  }
#endif
}

// The range of the inner node at (d, a) over the m sorted distinct keys
// (32 bytes each): [a, e), e the first position past a whose key shares fewer
// than d nibbles with key a.  A gallop from a, then a bisection: about
// 2 log2(e - a) keys read.
STL_HD uint32_t shamap_range_end(const uint8_t* skey, uint32_t m, uint32_t a, uint32_t d) {
  uint32_t ka[kShamapKeyWords], kb[kShamapKeyWords];
  shamap_load_key(ka, skey, a);
  uint32_t lo = a, hi = m;  // `lo` shares the d nibbles, `hi` does not (or is m)
  for (uint32_t step = 1;; step <<= 1) {
    const uint32_t p = a + step;
    if (p >= m) break;
    shamap_load_key(kb, skey, p);
    if (shamap_common_prefix(ka, kb) < d) {
      hi = p;
      break;
    }
    lo = p;
  }
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    shamap_load_key(kb, skey, mid);
    if (shamap_common_prefix(ka, kb) >= d) lo = mid; else hi = mid;
  }
  return hi;
}

// The first position of branch c of the node at depth d with range [a, e): the
// first key whose nibble d is c, or e when the branch is empty.  The hash of
// that branch is the slot of that position (the top of stl_shamap.hip).
STL_HD uint32_t shamap_branch_first(const uint8_t* skey, uint32_t a, uint32_t e, uint32_t d, uint32_t c) {
  uint32_t p0 = a, p1 = e;
  while (p0 < p1) {
    const uint32_t mid = p0 + ((p1 - p0) >> 1);
    if (shamap_nibble_bytes(skey + 32 * (size_t)mid, d) < c) p0 = mid + 1; else p1 = mid;
  }
  return (p0 < e && shamap_nibble_bytes(skey + 32 * (size_t)p0, d) == c) ? p0 : e;
}

// ---- what a stored inner node carries besides its hash (stl_shamap_nodes*) ----
// A node's ID: its first key with everything past the first d nibbles cleared
// (SHAMapNodeID's masked key), as memory-order dwords.
STL_HD void shamap_mask_key(uint32_t out[kShamapKeyWords], const uint32_t key[kShamapKeyWords], uint32_t d) {
  for (uint32_t i = 0; i < kShamapKeyWords; ++i) {
    const uint32_t keep = d <= 8u * i ? 0u : (d - 8u * i >= 8u ? 8u : d - 8u * i);  // nibbles of dword i that stay
    const uint32_t bytes = keep >> 1;
    uint32_t mask = bytes >= 4u ? 0xffffffffu : ((1u << (8u * bytes)) - 1u);
    if (keep & 1u) mask |= 0xf0u << (8u * bytes);
    out[i] = key[i] & mask;
  }
}

// The leaf rule: branch c of the node at depth d with range [a, e) holds one key
// (its hash is that key's leaf hash, not an inner node's) exactly when the
// branch's first position p (< e) is the range's last or the key after it
// parts from it at nibble d or before.  l: the neighbour bytes.
STL_HD bool shamap_branch_is_leaf(const int8_t* l, uint32_t p, uint32_t e, uint32_t d) {
  return p + 1 == e || (int32_t)l[p] <= (int32_t)d;
}

// The meta word of a stored node: bits 0-7 its depth, bit 16 + c: branch c is a leaf.
STL_HD uint32_t shamap_node_meta(uint32_t d, uint32_t leaf_mask) { return (d & 0xffu) | ((leaf_mask & 0xffffu) << 16); }

// SHA512Half of an inner node's record: rec[0] = kShamapInnerPrefix, rec[1 + 8 c
// .. 8 + 8 c] = the hash of branch c (zeros: empty), each as memory-order
// dwords -> out, 8 memory-order dwords.  Five compressions.
STL_HD void shamap_inner_hash(uint32_t out[kShamapKeyWords], const uint32_t* rec) {
  uint64_t st[8], w[16];
  sha512_init(st);
  for (uint32_t b = 0; b < 4; ++b) {
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) w[j] = be64_from_le32(rec[32 * b + 2 * j], rec[32 * b + 2 * j + 1]);
    sha512_compress(st, w);
  }
  // bytes 512 .. 515 of the message, the 0x80 that ends it, zeros, the bit length
  w[0] = be64_from_le32(rec[128], 0x80u);
#pragma unroll
  for (uint32_t j = 1; j < 15; ++j) w[j] = 0;
  w[15] = 516u * 8u;
  sha512_compress(st, w);
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    out[2 * j] = bswap32((uint32_t)(st[j] >> 32));
    out[2 * j + 1] = bswap32((uint32_t)st[j]);
  }
}

}  // namespace stl
