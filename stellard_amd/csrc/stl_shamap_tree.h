// stl_shamap_tree.h -- launch interface between stl_api_shamap_tree.cpp (host)
// and stl_shamap_tree.hip (gfx950 device code): the resident SHAMap
// (stl_shamap_tree_*), a state tree's root from each ledger's changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "stl_kernels.h"
#include "stl_shamap.h"

namespace stl {

// One generation of a tree: the sorted distinct keys and their leaf hashes
// (capacity * 32 bytes each), the 65,536 bucket values, and the meta words --
// [0] the item count, [8 .. 16) the root.
constexpr uint32_t kTreeMetaWords = 16, kTreeMetaRoot = 8;
struct TreeGen {
  uint8_t* key;
  uint8_t* leaf;
  uint32_t* bcnt;  // kTreeBuckets counts
  uint32_t* bh;    // kTreeBuckets hashes of 8 words
  uint32_t* meta;
};
// per generation besides the rows: 4 + 32 bytes per bucket and the meta words
size_t shamap_tree_gen_fixed_bytes();

// What an apply works in besides the two generations.
//   fixed: header and per-bucket words (shamap_tree_fixed_bytes)
//   batch: per row of the batch (kTreeBatchRowBytes): the compacted changes'
//          keys and leaf hashes, code bytes, positions, deltas and their scan
//   scratch: the dirty buckets' subtrees, per row of capacity
//          (kTreeScratchRowBytes) and a header: neighbour byte, key, hash slot
constexpr size_t kTreeBatchRowBytes = 32 + 32 + 4 + 4 + 4 + 4;
constexpr size_t kTreeScratchRowBytes = 1 + 32 + 32;
size_t shamap_tree_fixed_bytes();
size_t shamap_tree_batch_bytes(size_t n);
size_t shamap_tree_scratch_bytes(size_t capacity);

struct TreeApply {
  TreeGen from, to;        // the generation read and the one written: of one tree (an apply) or of two (a fork)
  uint32_t capacity;       // of the tree written: guards every store, sizes the scratch
  uint32_t from_capacity;  // of the tree read: clamps every read of `from` (shamap_tree_readable)
  uint32_t items_bound;    // host-known bound of the read generation's count: sizes the grids
  uint32_t after_bound;    // ... and of the count after the batch (the merge part), 1 .. capacity
  void* fixed;
  void* batch;
  void* scratch;
  void* sort_ws;           // the stream context's shamap workspace for n rows
  size_t temp_bytes;       // its temporary storage: >= shamap_temp_bytes(max(n, 65,536))
};

// One apply is two enqueues on `stream`, neither with a host wait.  key, leaf
// (or null: the key), op (or null: all sets): the batch of n >= 1 rows.
//   locate: steps 1 and 2 -- the distinct changes, their positions, deltas and
//           counts.  Writes the work areas alone.  Afterwards words [1] and [3]
//           of shamap_tree_change_counts (device memory) hold the inserted and
//           deleted keys: the count after the batch is the count + [1] - [3].
//   merge:  steps 3 to 7.  Writes a.to, the work areas and -- by the last
//           launch alone -- root (32 bytes) and counts (8 words, or null).
// fault / clock as launch_shamap_root; the marks: before the first launch (0),
// after sort and locate (1), the merge (2), the subtrees (3), the top and the
// finish (4).
hipError_t launch_shamap_tree_locate(const TreeApply& a, const uint8_t* key, const uint8_t* leaf, const uint8_t* op,
                                     uint32_t n, bool (*fault)(), const PhaseClock* clock, hipStream_t stream);
const uint32_t* shamap_tree_change_counts(void* fixed);
// emit (or null): the merge also stores the new tree's inner nodes of the
// dirty buckets (the scratch's level launches, emitting) and of the top
// prefixes above them, and its last launch writes their number to emit->count.
hipError_t launch_shamap_tree_merge(const TreeApply& a, uint32_t n, uint8_t* root, uint32_t* counts, bool (*fault)(),
                                    const PhaseClock* clock, hipStream_t stream, const ShamapEmit* emit = nullptr);
// root <- the generation's root; counts (or null) <- its item count and seven
// zeros; node_count (or null) <- zero: no node is stored.
hipError_t launch_shamap_tree_report(const TreeGen& g, uint8_t* root, uint32_t* counts, hipStream_t stream,
                                     uint32_t* node_count = nullptr);
// The snapshot: `from` (of a tree of from_capacity, its count at most
// items_bound <= capacity) copied into `to` (of a tree of `capacity`) -- rows by
// the count read on the device, the bucket values and the meta words -- and a
// finish launch that writes root, counts and node_count as the report does.
// Two launches, no sort, no hash, no host wait.
hipError_t launch_shamap_tree_snapshot(const TreeGen& from, uint32_t from_capacity, uint32_t items_bound,
                                       const TreeGen& to, uint32_t capacity, uint8_t* root, uint32_t* counts,
                                       uint32_t* node_count, bool (*fault)(), hipStream_t stream);
// The generation's sorted content -> key / leaf (either may be null) of `rows`
// rows, items_bound <= rows; *items (or null) <- the count.
hipError_t launch_shamap_tree_export(const TreeGen& g, uint32_t items_bound, uint8_t* key, uint8_t* leaf,
                                     uint32_t rows, uint32_t* items, hipStream_t stream);

}  // namespace stl
