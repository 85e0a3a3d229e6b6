// stl_shamap_get.h -- launch interface between stl_api_shamap_tree.cpp (host)
// and stl_shamap_get.hip (gfx950 device code): a resident SHAMap's nodes by
// node ID and its paths by key (stl_shamap_tree_get_nodes*).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "stl_shamap_tree.h"

namespace stl {

// The tasks a call can hold: a request has at most 80 rows, and none is stored
// at or past max_nodes.
uint32_t shamap_get_task_rows(size_t n, uint32_t max_nodes);

// A call's workspace: one scratch of `bound` rows (kTreeScratchRowBytes each and
// a header) with a word of 64 seen-bits per row, five words per task
// (shamap_get_task_rows: depth and position), four words per bucket (begin
// positions, marks, gathered counts and their scan), the tree's 4,369 top
// values with a seen word each, a 256-byte header and the scans' temporary
// storage (temp_bytes >= shamap_temp_bytes(max(n, 65,536))).  Nothing is sized
// by the tree's node count.  256-byte aligned.
size_t shamap_get_workspace_bytes(size_t bound, size_t tasks, size_t temp_bytes);

// The per-request arrays of a call (device pointers): id n * 32 bytes, depth n
// bytes, mode n bytes or null (every request FAT); status n bytes, first and
// rows n words, leaf_key / leaf_hash n * 32 bytes or null.
struct ShamapGet {
  const uint8_t* id;
  const uint8_t* depth;
  const uint8_t* mode;
  uint8_t* status;
  uint32_t* first;
  uint32_t* rows;
  uint8_t* leaf_key;
  uint8_t* leaf_hash;
};

// n >= 1 requests against generation g (of a tree of `cap` rows, its count at
// most `bound` <= cap) -> rq's answers and the node rows in emit, row
// first[i] + j the j-th node of request i, stored below emit.max_nodes only.
// All on `stream`, no host wait; the generation is not written.  emit.count and
// counts (8 words, or null) are written by the last launch alone.  fault /
// clock as launch_shamap_root; the marks: before the first launch (0), after
// the ranges, the tasks and the gather (1), the levels (2), the top and the
// finish (3, 4).
hipError_t launch_shamap_tree_get_nodes(const TreeGen& g, uint32_t cap, uint32_t bound, const ShamapGet& rq, uint32_t n,
                                        const ShamapEmit& emit, uint32_t* counts, void* ws, size_t temp_bytes,
                                        bool (*fault)(), const PhaseClock* clock, hipStream_t stream);

}  // namespace stl
