// stl_shamap_lookup_core.h -- the rules of the resident SHAMap's read-only
// calls (stl_shamap_tree_lookup*, stl_shamap_tree_compare*): what the device
// kernels (stl_shamap_lookup.hip) and the host emulation
// (tests/native/hostemu_shamap_lookup.cpp) share.
//
// A generation's keys are sorted and its 65,536 bucket counts are kept, so the
// keys of bucket b are the positions [begin[b], begin[b] + bcnt[b]) with begin
// the exclusive scan of bcnt.  A lookup bisects that range alone.  A compare
// takes a bucket whose (count, hash) is equal in both trees as equal -- a leaf
// hash commits to its key, so equal bucket hashes mean equal content, the
// assumption SHAMap::compare makes branch by branch -- and merges the two
// ranges of every other bucket by rank: each item finds its place among the
// other tree's keys of the same bucket, so the slots of one bucket are written
// exactly once each, in key order, without a sort.
#pragma once
#include "stl_shamap_tree_core.h"

namespace stl {

// the kinds of a difference (STL_SHAMAP_DIFF_* of include/stl.h); 0: none
constexpr uint32_t kDiffNone = 0, kDiffAOnly = 1, kDiffBOnly = 2, kDiffChanged = 3;
constexpr uint32_t kDiffNoRow = 0xffffffffu;  // a slot's source row in the tree that lacks the key

// A bucket's range in a generation of m items, whatever the counts say: never past m.
STL_HD void shamap_lookup_range(uint32_t begin, uint32_t cnt, uint32_t m, uint32_t* lo, uint32_t* hi) {
  *lo = begin < m ? begin : m;
  *hi = cnt < m - *lo ? *lo + cnt : m;
}

// The in-bucket search: the first position in [lo, hi) of the sorted keys whose
// key is not below `key` (hi: none); *found: that key equals it.
STL_HD uint32_t shamap_lookup_lower_bound(const uint8_t* skey, uint32_t lo, uint32_t hi,
                                          const uint32_t key[kShamapKeyWords], bool* found) {
  const uint32_t end = hi;
  uint32_t k[kShamapKeyWords];
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    shamap_load_key(k, skey, mid);
    if (shamap_key_less(k, key)) lo = mid + 1; else hi = mid;
  }
  *found = false;
  if (lo < end) {
    shamap_load_key(k, skey, lo);
    *found = shamap_common_prefix(k, key) == 64u;
  }
  return lo;
}

// The bucket-differs rule: the buckets' values (count, hash) are not the same.
STL_HD bool shamap_bucket_differs(uint32_t cnt_a, const uint32_t* h_a, uint32_t cnt_b, const uint32_t* h_b) {
  if (cnt_a != cnt_b) return true;
  for (uint32_t i = 0; i < kShamapKeyWords; ++i)
    if (h_a[i] != h_b[i]) return true;
  return false;
}

// The merged rank of an item within its bucket's cnt_a + cnt_b slots.  Item i
// of A's range (0-based within the bucket) with lb_b keys of B's range below
// its own goes to i + lb_b; item j of B's range with ub_a keys of A's range not
// above its own goes to j + ub_a.  Of a key in both, A's item comes first
// (i + j, then j + i + 1), and the ranks of a bucket are a permutation of
// 0 .. cnt_a + cnt_b - 1.
STL_HD uint32_t shamap_diff_rank_a(uint32_t i, uint32_t lb_b) { return i + lb_b; }
STL_HD uint32_t shamap_diff_rank_b(uint32_t j, uint32_t ub_a) { return j + ub_a; }

// What a slot reports.  An A item: A_ONLY when B lacks its key, CHANGED when
// B's leaf hash differs, nothing when it is equal.  A B item: B_ONLY when A
// lacks its key, else nothing -- the A side reports a matched pair.
STL_HD uint32_t shamap_diff_kind_a(bool found_in_b, bool leaf_equal) {
  return !found_in_b ? kDiffAOnly : (leaf_equal ? kDiffNone : kDiffChanged);
}
STL_HD uint32_t shamap_diff_kind_b(bool found_in_a) { return found_in_a ? kDiffNone : kDiffBOnly; }

// The bucket that holds slot p: the last b with off[b] <= p, over the exclusive
// scan `off` of the buckets' slot counts (p below their total).  Buckets without
// slots share their successor's offset, so the last one at an offset is the one
// with slots.
STL_HD uint32_t shamap_diff_bucket_of(const uint32_t* off, uint32_t p) {
  uint32_t lo = 0, hi = kTreeBuckets;  // the first bucket whose offset is past p
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= p) lo = mid + 1; else hi = mid;
  }
  return lo - 1;  // off[0] = 0 <= p
}

// One slot of a compare.  ka / kb: the two generations' sorted keys; la / lb
// their leaf hashes; [a0, a1) and [b0, b1) the bucket's ranges; q: the slot's
// number within the bucket as the grid hands it out (A's items first, then B's).
// Returns the merged rank; *kind, *row_a, *row_b: what goes into that rank's slot.
STL_HD uint32_t shamap_diff_slot(const uint8_t* ka, const uint8_t* la, uint32_t a0, uint32_t a1, const uint8_t* kb,
                                 const uint8_t* lb, uint32_t b0, uint32_t b1, uint32_t q, uint32_t* kind,
                                 uint32_t* row_a, uint32_t* row_b) {
  const uint32_t cnt_a = a1 - a0;
  uint32_t key[kShamapKeyWords], x[kShamapKeyWords], y[kShamapKeyWords];
  bool found = false;
  if (q < cnt_a) {
    const uint32_t i = a0 + q;
    shamap_load_key(key, ka, i);
    const uint32_t p = shamap_lookup_lower_bound(kb, b0, b1, key, &found);
    bool equal = false;
    if (found) {
      shamap_load_key(x, la, i);
      shamap_load_key(y, lb, p);
      equal = shamap_common_prefix(x, y) == 64u;
    }
    *kind = shamap_diff_kind_a(found, equal);
    *row_a = i;
    *row_b = found ? p : kDiffNoRow;
    return shamap_diff_rank_a(q, p - b0);
  }
  const uint32_t j = b0 + (q - cnt_a);
  shamap_load_key(key, kb, j);
  const uint32_t p = shamap_lookup_lower_bound(ka, a0, a1, key, &found);
  *kind = shamap_diff_kind_b(found);
  *row_a = found ? p : kDiffNoRow;
  *row_b = j;
  return shamap_diff_rank_b(q - cnt_a, (p - a0) + (found ? 1u : 0u));  // keys of A not above this one
}

}  // namespace stl
