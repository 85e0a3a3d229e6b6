// stl_shamap_tree_core.h -- the rules of the resident SHAMap (stl_shamap_tree_*):
// what the device kernels (stl_shamap_tree.hip) and the host emulation
// (tests/native/hostemu_shamap_tree.cpp) share.
//
// The tree's keys fall into 16^T buckets by their first T = 4 nibbles.  Every
// nibble prefix p of length <= T has a value (cnt, h): cnt the keys under p;
// h zero for cnt = 0, the one key's leaf hash for cnt = 1, the hash of the
// inner node at (len p, p) for cnt >= 2.  A bucket's value depends on the
// bucket's keys alone (for cnt >= 2 it is what the level kernel of
// stl_shamap.hip leaves in the slot of the bucket's first key after depths 63
// down to T); a shorter prefix's value follows from its 16 children's values
// (shamap_tree_top_value), and the root is the inner hash over the 16 depth-1
// values whenever the tree holds a key.  So a batch of changes rehashes the
// buckets it touches and the 4,369 nodes above the buckets, nothing else.
#pragma once
#include "stl_shamap_core.h"

namespace stl {

constexpr uint32_t kTreeBucketDepth = 4;
constexpr uint32_t kTreeBuckets = 1u << (4 * kTreeBucketDepth);  // 65,536
// the values of the prefixes of length 3, 2, 1 (4,096 + 256 + 16) sit one after another
constexpr uint32_t kTreeTopValues = 4096 + 256 + 16;

// change codes (one per distinct change): what the row asks and what the tree holds
constexpr uint32_t kTreeOpDelete = 1u, kTreeFound = 2u;

// The bucket of a key: its first four nibbles, big-endian.
STL_HD uint32_t shamap_tree_bucket(const uint32_t key[kShamapKeyWords]) {
  return ((key[0] & 0xffu) << 8) | ((key[0] >> 8) & 0xffu);
}

// How many rows of a generation may be read: its stated count, and never more
// than the capacity its arrays were made for.  A fork reads one tree's
// generation and writes another's, so the reading side has a capacity of its
// own; every read of `from` goes by this, every store by the writing side's.
STL_HD uint32_t shamap_tree_readable(uint32_t stated_count, uint32_t from_capacity) {
  return stated_count < from_capacity ? stated_count : from_capacity;
}

// The rows a snapshot copies: what may be read, and never more than the
// written side holds (the host refuses a snapshot that would not fit).
STL_HD uint32_t shamap_tree_snapshot_rows(uint32_t stated_count, uint32_t from_capacity, uint32_t to_capacity) {
  const uint32_t m = shamap_tree_readable(stated_count, from_capacity);
  return m < to_capacity ? m : to_capacity;
}

// The last-of-equals head rule over the batch's sorted positions: position i
// holds a change when the key after it differs (or there is none).  The sort is
// stable, so of equal keys this is the highest row: the batch reads as a
// sequence of changes.
STL_HD bool shamap_tree_head(bool is_last_position, uint32_t common_prefix_with_next) {
  return is_last_position || common_prefix_with_next < 64u;
}

// What a change does to the item count: +1 for a set of an absent key, -1 for
// a delete of a present one, else 0.
STL_HD int32_t shamap_tree_delta(bool is_delete, bool found) {
  if (is_delete) return found ? -1 : 0;
  return found ? 0 : 1;
}

// Where things land in the other generation.  scan_before: the sum of the
// deltas of the changes whose keys are smaller (the exclusive scan).  A
// resident item i that is not deleted keeps its place among the survivors and
// the insertions before it; an inserted change goes behind the resident items
// below its position pos (the first resident key >= its own).
STL_HD uint32_t shamap_tree_item_dest(uint32_t i, uint32_t scan_before) { return i + scan_before; }
STL_HD uint32_t shamap_tree_insert_dest(uint32_t pos, uint32_t scan_before) { return pos + scan_before; }

// The change that bears on resident item i, from the changes' positions alone.
// pos[0 .. k) ascends with the changes' keys; pos[j] < i means key j is smaller
// than item i's, pos[j] == i that it is smaller or (found) equal, and the equal
// one is the last of those.  Returns r, the changes with smaller keys, and
// *hit: change r has item i's key.
STL_HD uint32_t shamap_tree_changes_before(const uint32_t* pos, const uint8_t* code, uint32_t k, uint32_t i,
                                           bool* hit) {
  uint32_t lo = 0, hi = k;  // the first j with pos[j] > i
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (pos[mid] <= i) lo = mid + 1; else hi = mid;
  }
  *hit = lo > 0 && pos[lo - 1] == i && (code[lo - 1] & kTreeFound);
  return *hit ? lo - 1 : lo;
}

// The first position in the m sorted keys (32 bytes each) whose key is not
// below `key`; *found: that key equals it.
STL_HD uint32_t shamap_tree_lower_bound(const uint8_t* skey, uint32_t m, const uint32_t key[kShamapKeyWords],
                                        bool* found) {
  uint32_t lo = 0, hi = m;
  uint32_t k[kShamapKeyWords];
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    shamap_load_key(k, skey, mid);
    if (shamap_key_less(k, key)) lo = mid + 1; else hi = mid;
  }
  *found = false;
  if (lo < m) {
    shamap_load_key(k, skey, lo);
    *found = shamap_common_prefix(k, key) == 64u;
  }
  return lo;
}

// The first position whose key's bucket is not below b (b = kTreeBuckets: m).
STL_HD uint32_t shamap_tree_bucket_begin(const uint8_t* skey, uint32_t m, uint32_t b) {
  uint32_t lo = 0, hi = m;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint8_t* p = skey + 32 * (size_t)mid;
    if ((((uint32_t)p[0] << 8) | p[1]) < b) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The top recurrence: the value of a prefix shorter than T from its 16
// children's values (cnt[c], h + 8 c).  `root`: the prefix is empty -- the root
// is an inner node whatever it holds.  Returns the count; out: the hash.
STL_HD uint32_t shamap_tree_top_value(const uint32_t* cnt, const uint32_t* h, bool root,
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
    uint32_t rec[kShamapRecordWords];
    rec[0] = kShamapInnerPrefix;
    for (uint32_t c = 0; c < kShamapBranches; ++c)
      for (uint32_t i = 0; i < kShamapKeyWords; ++i) rec[1 + 8 * c + i] = cnt[c] ? h[8 * c + i] : 0u;
    shamap_inner_hash(out, rec);
  }
  return sum;
}

// ---- the top nodes an apply stores (stl_shamap_tree_apply_nodes*) ----
// A prefix shorter than T is stored when a dirty bucket lies below it and it is
// an inner node: it holds two keys or more, or it is the root and holds one.
STL_HD bool shamap_tree_top_emits(uint32_t cnt, bool root, bool dirty_below) {
  return dirty_below && (cnt >= 2u || (root && cnt >= 1u));
}

// The stored form of the prefix numbered t among those of length `depth`
// (0 .. T - 1) from its 16 children's values: the body (the 16 hashes, zeros
// for an empty child), the ID (the prefix's nibbles, then zeros) and the leaf
// mask (the children that hold one key).
STL_HD uint32_t shamap_tree_top_node(const uint32_t* cnt, const uint32_t* h, uint32_t depth, uint32_t t,
                                     uint32_t body[16 * kShamapKeyWords], uint32_t id[kShamapKeyWords]) {
  uint32_t leaf = 0;
  for (uint32_t c = 0; c < kShamapBranches; ++c) {
    if (cnt[c] == 1u) leaf |= 1u << c;
    for (uint32_t i = 0; i < kShamapKeyWords; ++i) body[8 * c + i] = cnt[c] ? h[8 * c + i] : 0u;
  }
  const uint32_t v = depth ? t << (4u * (kTreeBucketDepth - depth)) : 0u;  // the prefix, left-aligned in 16 bits
  id[0] = ((v >> 8) & 0xffu) | ((v & 0xffu) << 8);
  for (uint32_t i = 1; i < kShamapKeyWords; ++i) id[i] = 0;
  return leaf;
}

}  // namespace stl
