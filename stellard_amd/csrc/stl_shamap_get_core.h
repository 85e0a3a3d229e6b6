// stl_shamap_get_core.h -- the rules of the resident SHAMap's answers by node ID
// (stl_shamap_tree_get_nodes*: SHAMap::getNodeFat and SHAMap::getPath): what the
// device kernels (stl_shamap_get.hip) and the host emulation
// (tests/native/hostemu_shamap_get.cpp) share.
//
// Everything follows from key ranges.  The node at (depth, id) covers the keys
// [lo, hi) whose first `depth` nibbles are id's; with c = hi - lo it is an inner
// node when c >= 2 (or it is the root and c == 1), a leaf when c == 1 and the
// range one nibble shorter holds two keys or more (or depth == 1), the empty
// root when depth == 0 and c == 0, and absent otherwise.  An inner node is named
// by (its depth, the position of its first key) -- the name the level kernel of
// stl_shamap.hip hashes it under -- so a request's rows are a list of such pairs,
// known before anything is hashed:
//   NODE  the node itself
//   FAT   the nodes along id at depths depth .. L, L the nibbles the range's
//         first and last key share (the chain of nodes with one inner child
//         that getNodeFat's do-while follows), then the inner children of the
//         node at L in branch order
//   PATH  the inner nodes along the key at depths 0 .. D - 1, D the first depth
//         at which fewer than two keys share the key's prefix (at least 1)
#pragma once
#include "stl_shamap_lookup_core.h"

namespace stl {

// the modes and the answers (STL_SHAMAP_GET_* / STL_SHAMAP_AT_* of include/stl.h)
constexpr uint32_t kGetNode = 0, kGetFat = 1, kGetPath = 2;
constexpr uint32_t kAtAbsent = 0, kAtInner = 1, kAtLeaf = 2, kAtEmptyRoot = 3, kAtInvalid = 4, kAtOtherLeaf = 5;
constexpr uint32_t kGetMaxRows = 80;          // 64 nodes of a chain and 16 children
constexpr uint32_t kGetNoLeaf = 0xffffffffu;  // no leaf to report

// What a request reads of a generation: the sorted keys, the bucket counts and
// their exclusive scan, and m, the rows that may be read (shamap_tree_readable).
struct GetTree {
  const uint8_t* key;
  const uint32_t* begin;
  const uint32_t* bcnt;
  uint32_t m;
};

// SHAMapNodeID(depth, id) as it comes off the wire is not masked: an id with a
// bit set past its first `depth` nibbles names no node.
STL_HD bool shamap_get_id_masked(const uint32_t id[kShamapKeyWords], uint32_t depth) {
  uint32_t k[kShamapKeyWords];
  shamap_mask_key(k, id, depth);
  return shamap_common_prefix(k, id) == 64u;
}

// The kind of node at (depth, id) from the size c of its range;
// parent_two: the range one nibble shorter holds two keys or more.
STL_HD uint32_t shamap_get_kind(uint32_t c, uint32_t depth, bool parent_two) {
  if (c >= 2u || (depth == 0 && c == 1u)) return kAtInner;
  if (depth == 0) return kAtEmptyRoot;
  if (c == 1u && (depth == 1u || parent_two)) return kAtLeaf;
  return kAtAbsent;
}

// The depth at which a path ends, from the two longest prefixes the key shares
// with any key of the tree (-1: there is no such key): at every depth up to the
// second longest, two keys share the key's prefix.  The root is always a node.
STL_HD uint32_t shamap_get_path_depth(int32_t second) { return second < 0 ? 1u : (uint32_t)second + 1u; }

// ... and what sits there: the key with the longest shared prefix `best`, if it
// reaches depth D.
STL_HD uint32_t shamap_get_path_status(int32_t best, uint32_t D) {
  if (best < (int32_t)D) return kAtAbsent;
  return best == 64 ? kAtLeaf : kAtOtherLeaf;
}

// The range [lo, hi) of the masked id at `depth` (0 .. 63).  Above the bucket
// depth it is read off the begins of the prefix's first and last bucket; at or
// below it the id's bucket is bisected.
STL_HD void shamap_get_range(const GetTree& t, const uint32_t id[kShamapKeyWords], uint32_t depth, uint32_t* lo,
                             uint32_t* hi) {
  const uint32_t b0 = shamap_tree_bucket(id);
  if (depth < kTreeBucketDepth) {
    uint32_t b1 = b0 + (1u << (4u * (kTreeBucketDepth - depth))) - 1u;
    if (b1 > kTreeBuckets - 1u) b1 = kTreeBuckets - 1u;  // never for a masked id: its bucket ends in zeros
    uint32_t x, y;
    shamap_lookup_range(t.begin[b0], t.bcnt[b0], t.m, lo, &x);
    shamap_lookup_range(t.begin[b1], t.bcnt[b1], t.m, &y, hi);
    if (*hi < *lo) *hi = *lo;  // never, while the counts describe the keys
    return;
  }
  uint32_t blo, bhi;
  shamap_lookup_range(t.begin[b0], t.bcnt[b0], t.m, &blo, &bhi);
  bool found = false;
  const uint32_t p = shamap_lookup_lower_bound(t.key, blo, bhi, id, &found);
  *lo = *hi = p;
  if (p >= bhi) return;
  uint32_t k[kShamapKeyWords];
  shamap_load_key(k, t.key, p);
  if (shamap_common_prefix(k, id) >= depth) *hi = shamap_range_end(t.key, bhi, p, depth);
}

// The first position past p in [p, hi) whose nibble d is above key p's: the end
// of key p's branch of the node at depth d with range [.., hi).
STL_HD uint32_t shamap_get_branch_end(const uint8_t* skey, uint32_t p, uint32_t hi, uint32_t d) {
  const uint32_t nib = shamap_nibble_bytes(skey + 32 * (size_t)p, d);
  uint32_t lo = p + 1;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (shamap_nibble_bytes(skey + 32 * (size_t)mid, d) <= nib) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One request.  Returns the status; *rows: its node rows; *leaf_pos: the
// position of the leaf to report, or kGetNoLeaf.  With `nodes`, emit(j, d, pos)
// is called for row j = 0 .. rows - 1 in order: the inner node at depth d whose
// first key is at position pos.  Without, only the count is made (a path's
// positions cost a bisection each).  depth is not looked at for a path.
template <class Emit>
STL_HD uint32_t shamap_get_request(const GetTree& t, const uint32_t id[kShamapKeyWords], uint32_t depth, uint32_t mode,
                                   bool nodes, Emit&& emit, uint32_t* rows, uint32_t* leaf_pos) {
  *rows = 0;
  *leaf_pos = kGetNoLeaf;
  uint32_t k[kShamapKeyWords], k2[kShamapKeyWords];
  if (mode > kGetPath) return kAtInvalid;
  if (mode == kGetPath) {
    if (t.m == 0) return kAtAbsent;
    uint32_t blo, bhi;
    const uint32_t b = shamap_tree_bucket(id);
    shamap_lookup_range(t.begin[b], t.bcnt[b], t.m, &blo, &bhi);
    bool found = false;
    const uint32_t p = shamap_lookup_lower_bound(t.key, blo, bhi, id, &found);  // where the key is, or would go
    // the keys that share the most with it are the two either side of that place
    int32_t best = -1, second = -1;
    uint32_t best_pos = kGetNoLeaf;
    for (uint32_t o = 0; o < 4u; ++o) {
      if (p + o < 2u || p + o - 2u >= t.m) continue;
      const uint32_t q = p + o - 2u;
      shamap_load_key(k, t.key, q);
      const int32_t cp = (int32_t)shamap_common_prefix(k, id);
      if (cp > best) {
        second = best;
        best = cp;
        best_pos = q;
      } else if (cp > second) {
        second = cp;
      }
    }
    if (second > 63) second = 63;  // never: the keys are distinct
    const uint32_t D = shamap_get_path_depth(second);
    *rows = D;
    if (nodes) {
      uint32_t lo = 0;
      const uint32_t hi = p < t.m ? p + 1u : t.m;
      for (uint32_t d = 0; d < D; ++d) {
        shamap_mask_key(k, id, d);
        lo = shamap_lookup_lower_bound(t.key, lo, hi, k, &found);  // the first key under the key's d nibbles
        emit(d, d, lo);
      }
    }
    const uint32_t st = shamap_get_path_status(best, D);
    if (st != kAtAbsent) *leaf_pos = best_pos;
    return st;
  }
  if (depth >= kShamapDepths) return kAtInvalid;
  if (!shamap_get_id_masked(id, depth)) return kAtAbsent;
  uint32_t lo, hi;
  shamap_get_range(t, id, depth, &lo, &hi);
  const uint32_t c = hi - lo;
  bool parent_two = false;
  if (c == 1u && depth >= 2u) {
    shamap_load_key(k, t.key, lo);
    if (lo > 0) {
      shamap_load_key(k2, t.key, lo - 1u);
      parent_two = shamap_common_prefix(k, k2) >= depth - 1u;
    }
    if (!parent_two && lo + 1u < t.m) {
      shamap_load_key(k2, t.key, lo + 1u);
      parent_two = shamap_common_prefix(k, k2) >= depth - 1u;
    }
  }
  const uint32_t st = shamap_get_kind(c, depth, parent_two);
  if (st == kAtLeaf) *leaf_pos = lo;
  if (st != kAtInner) return st;
  if (mode == kGetNode || c == 1u) {
    *rows = 1;
    if (nodes) emit(0u, depth, lo);
    return st;
  }
  shamap_load_key(k, t.key, lo);
  shamap_load_key(k2, t.key, hi - 1u);
  uint32_t L = shamap_common_prefix(k, k2);
  if (L < depth) L = depth;                          // never: both keys share the id's nibbles
  if (L > kShamapDepths - 1u) L = kShamapDepths - 1u;  // never: the keys are distinct
  uint32_t j = 0;
  for (uint32_t d = depth; d <= L; ++d, ++j)
    if (nodes) emit(j, d, lo);
  if (L + 1u < kShamapDepths) {
    uint32_t branches = 0;
    for (uint32_t p = lo; p < hi && branches < kShamapBranches; ++branches) {
      const uint32_t q = shamap_get_branch_end(t.key, p, hi, L);
      if (q - p >= 2u) {
        if (nodes) emit(j, L + 1u, p);
        ++j;
      }
      p = q;
    }
  }
  *rows = j;
  return st;
}

// The scratch position of generation position pos, whose bucket b was gathered:
// the gather keeps a bucket's keys together and in order.
STL_HD uint32_t shamap_get_scratch_pos(uint32_t pos, uint32_t begin_b, uint32_t off_b) {
  return off_b + (pos - begin_b);
}

// The top value (of the prefixes of length 3, 2, 1 and the root, one after
// another) that holds prefix t of length d < 4, and where its 16 children's
// values begin: in the same array, or for d == 3 among the bucket values.
STL_HD uint32_t shamap_get_top_index(uint32_t d, uint32_t t) {
  return d == 3u ? t : d == 2u ? 4096u + t : d == 1u ? 4096u + 256u + t : kTreeTopValues;
}

}  // namespace stl
