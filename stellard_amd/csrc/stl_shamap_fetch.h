// stl_shamap_fetch.h -- launch interface between stl_api_shamap_tree.cpp (host)
// and stl_shamap_fetch.hip (gfx950 device code): the fetch pack of one resident
// SHAMap against another (stl_shamap_tree_fetch_pack*).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "stl_shamap_tree.h"

namespace stl {

// A fetch pack's workspace: a scratch of want_bound rows and one of have_bound
// rows (kTreeScratchRowBytes each: neighbour byte, key, hash slot, and a
// header), six words per bucket (the two begin positions, the two row counts
// and their scans), both trees' 4,369 top values, a 256-byte header and the
// scans' temporary storage (temp_bytes >= shamap_temp_bytes(65,536)).  Nothing
// is sized by the number of nodes.  256-byte aligned.
size_t shamap_fetch_workspace_bytes(size_t want_bound, size_t have_bound, size_t temp_bytes);

// The inner nodes of generation `want` (of a tree of cap_want rows) that `have`
// (cap_have; null: no tree, every inner node of want) does not hold at the same
// ID with the same hash -> emit, numbered freely, stored below emit.max_nodes
// only.  want_bound / have_bound: host-known bounds of the two item counts,
// which size the grids and the scratches (have_bound is not read without have).
// All on `stream`, no host wait; neither generation is written.  emit.count and
// counts (8 words, or null) are written by the last launch alone.  fault / clock
// as launch_shamap_root; the marks: before the first launch (0), after the
// buckets and the gather (1), the levels (2), the top and the finish (3, 4).
hipError_t launch_shamap_tree_fetch_pack(const TreeGen& want, uint32_t cap_want, uint32_t want_bound,
                                         const TreeGen* have, uint32_t cap_have, uint32_t have_bound,
                                         const ShamapEmit& emit, uint32_t* counts, void* ws, size_t temp_bytes,
                                         bool (*fault)(), const PhaseClock* clock, hipStream_t stream);

}  // namespace stl
