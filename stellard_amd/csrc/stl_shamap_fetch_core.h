// stl_shamap_fetch_core.h -- the rules of a fetch pack between two resident
// SHAMaps (stl_shamap_tree_fetch_pack*): what the device kernels
// (stl_shamap_fetch.hip) and the host emulation
// (tests/native/hostemu_shamap_fetch.cpp) share.
//
// The pack of `want` against `have` is every inner node of want, at
// SHAMapNodeID (depth, masked key), for which have holds no inner node at the
// same ID with the same hash -- the set SHAMap::getFetchPack's walk visits, which
// descends into a child only when !have->hasInnerNode(childID, childHash).  The
// test is by position: a node of want whose hash have holds at another ID is in
// the pack.
//
// Below the buckets (depth >= 4) a bucket whose (count, hash) is equal in both
// trees is not examined (shamap_bucket_differs, the compare's rule); of the
// others want's keys are gathered where it holds an inner node (two keys or
// more), and have's where both do.  Both scratches are hashed level by level,
// have first at every depth, so that the slot of a have node's first key holds
// that node's hash when want's nodes of the same depth ask for it.  Above the
// buckets every prefix of both trees is folded and compared.
#pragma once
#include "stl_shamap_lookup_core.h"

namespace stl {

// The keys a differing bucket sends to want's scratch: all of them when they
// make an inner node at depth 4, none otherwise.
STL_HD uint32_t shamap_fetch_want_rows(bool differs, uint32_t cnt_want) {
  return differs && cnt_want >= 2u ? cnt_want : 0u;
}

// ... and to have's: only where want asks and have holds an inner node too.
STL_HD uint32_t shamap_fetch_have_rows(bool differs, uint32_t cnt_want, uint32_t cnt_have) {
  return differs && cnt_want >= 2u && cnt_have >= 2u ? cnt_have : 0u;
}

// hasInnerNode(id, hash) over a scratch whose level launches have just run depth
// d: hkey the mh gathered keys in order, hl their neighbour bytes, hslot the hash
// slots.  id: the asking node's first key masked to d nibbles, so the lower
// bound p is the first key under that prefix, if any.  have holds an inner node
// there exactly when key p shares the d nibbles and starts a node at depth d;
// its hash is then slot p.
STL_HD bool shamap_fetch_have_holds(const uint8_t* hkey, const int8_t* hl, const uint8_t* hslot, uint32_t mh,
                                    const uint32_t id[kShamapKeyWords], uint32_t d,
                                    const uint32_t hash[kShamapKeyWords]) {
  if (mh == 0) return false;
  bool found = false;
  const uint32_t p = shamap_lookup_lower_bound(hkey, 0, mh, id, &found);
  if (p >= mh) return false;
  uint32_t k[kShamapKeyWords];
  shamap_load_key(k, hkey, p);
  if (shamap_common_prefix(k, id) < d) return false;
  if (!shamap_starts_node(p ? (int32_t)hl[p - 1] : -1, (int32_t)hl[p], (int32_t)d)) return false;
  shamap_load_key(k, hslot, p);
  return shamap_common_prefix(k, hash) == 64u;
}

// shamap_tree_top_value with the 129-word record in storage the caller names
// (the kernel's LDS, so that no lane keeps it in private memory): the value of
// a prefix shorter than the bucket depth from its 16 children's values.  After
// a call that hashed, rec[1 .. 129) is the node's body.
STL_HD uint32_t shamap_fetch_top_value(const uint32_t* cnt, const uint32_t* h, bool root, uint32_t* rec,
                                       uint32_t out[kShamapKeyWords]) {
  uint32_t sum = 0, one = 0;
  for (uint32_t c = 0; c < kShamapBranches; ++c) {
    sum += cnt[c];
    if (cnt[c]) one = c;
  }
  if (sum == 0) {
    for (uint32_t i = 0; i < kShamapKeyWords; ++i) out[i] = 0;
  } else if (sum == 1 && !root) {
    for (uint32_t i = 0; i < kShamapKeyWords; ++i) out[i] = h[8 * one + i];
  } else {
    rec[0] = kShamapInnerPrefix;
    for (uint32_t c = 0; c < kShamapBranches; ++c)
      for (uint32_t i = 0; i < kShamapKeyWords; ++i) rec[1 + 8 * c + i] = cnt[c] ? h[8 * c + i] : 0u;
    shamap_inner_hash(out, rec);
  }
  return sum;
}

// A prefix shorter than the bucket depth is an inner node when it holds two
// keys or more, or is the root and holds one.
STL_HD bool shamap_fetch_top_inner(uint32_t cnt, bool root) { return cnt >= 2u || (root && cnt >= 1u); }

// ... and goes into the pack when have's value of the same prefix is no inner
// node or hashes differently.  Only asked for a prefix that is an inner node of want.
STL_HD bool shamap_fetch_top_keeps(const uint32_t h_want[kShamapKeyWords], uint32_t cnt_have,
                                   const uint32_t h_have[kShamapKeyWords], bool root) {
  if (!shamap_fetch_top_inner(cnt_have, root)) return true;
  return shamap_common_prefix(h_want, h_have) != 64u;
}

}  // namespace stl
