// stl_shamap_lookup.h -- launch interface between stl_api_shamap_tree.cpp (host)
// and stl_shamap_lookup.hip (gfx950 device code): the resident SHAMap's
// read-only calls, lookup by key (stl_shamap_tree_lookup*) and the difference
// of two trees (stl_shamap_tree_compare*).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "stl_shamap_tree.h"

namespace stl {

// A lookup's workspace: the 65,536 bucket begin positions and the scan's
// temporary storage (temp_bytes >= shamap_temp_bytes(65,536)); 256-byte aligned.
size_t shamap_lookup_workspace_bytes(size_t temp_bytes);

// n >= 1 keys (32 bytes each, 16-byte aligned) against generation g of a tree
// of `capacity` rows; the item count is read on the device.  words: ceil(n / 64)
// words, written whole; leaf (or null): n * 32 bytes, 16-byte aligned; position
// (or null): n words.  buckets: false bisects the whole array instead of the
// key's bucket (the A/B variant of tools/shamap_lookup_bench.py).  Two enqueues
// (the scan of the bucket counts, the lookup kernel), no host wait.  fault (or
// null): asked before every HIP call; true makes the call fail there.
hipError_t launch_shamap_tree_lookup(const TreeGen& g, uint32_t capacity, const uint8_t* key, uint32_t n,
                                     uint64_t* words, uint8_t* leaf, uint32_t* position, bool buckets, void* ws,
                                     size_t temp_bytes, bool (*fault)(), hipStream_t stream);

// Where a compare writes (stl_shamap_diff_out of include/stl.h, device pointers).
struct ShamapDiff {
  uint8_t* key;
  uint8_t* kind;
  uint8_t* leaf_a;
  uint8_t* leaf_b;
  uint32_t max_rows;
  uint32_t* counts;  // 8 words: written by the finish launch alone
};

// A compare's workspace per slot -- an item of a bucket that differs, of either
// tree: its flag word, the flags' scan, and its source rows in a and in b -- and
// besides: four words per bucket (the two begin positions, the slot count and
// its scan), a 256-byte header and the scans' temporary storage (temp_bytes >=
// shamap_temp_bytes(max(slots, 65,536))).
constexpr size_t kShamapDiffSlotBytes = 4 + 4 + 4 + 4;
size_t shamap_compare_workspace_bytes(size_t slots, size_t temp_bytes);

// The differences of generation a (capacity cap_a) and b (cap_b) -> out, in key
// order; slots: a host-known bound of the two item counts' sum, which sizes the
// grids and the workspace (0: both trees are known to be empty).  All on
// `stream`, no host wait; out.counts is written by the last launch alone and no
// store goes past out.max_rows rows.
hipError_t launch_shamap_tree_compare(const TreeGen& a, uint32_t cap_a, const TreeGen& b, uint32_t cap_b,
                                      uint32_t slots, const ShamapDiff& out, void* ws, size_t temp_bytes,
                                      bool (*fault)(), hipStream_t stream);

}  // namespace stl
