// stl_shamap.h -- launch interface between stl_api_shamap.cpp (host) and
// stl_shamap.hip (gfx950 device code): the SHAMap root of a set of keys
// (stl_shamap_root*).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "stl_kernels.h"

namespace stl {

// Workspace bytes per row besides the sort's own temporary storage: two 8-byte
// sort words, two 4-byte row numbers (the sort's double buffers; the scan's
// flags and the compacted rows reuse them), the neighbour byte, the sorted
// keys and the hash slots (32 bytes each).
constexpr size_t kShamapRowBytes = 8 + 8 + 4 + 4 + 1 + 32 + 32;
constexpr size_t kShamapHeaderBytes = 512;  // 64 nodes-per-depth words, distinct and selected counts
constexpr uint32_t kShamapHdrDistinct = 64;  // the header word that holds the number of sorted distinct keys
constexpr uint32_t kShamapHdrEmitted = 66;   // ... and the one that numbers the stored nodes (stl_shamap_nodes*)

// Where a call stores its inner nodes (stl_shamap_nodes_out of include/stl.h,
// device pointers): row i of hash (32 B), body (512 B), id (32 B, or null) and
// meta (a word, or null), i < max_nodes; hash, body and id 16-byte aligned.
// Rows are numbered by adding to one header word, so their order is free.
constexpr size_t kShamapNodeRowBytes = 32 + 512 + 32 + 4;
struct ShamapEmit {
  uint8_t* hash;
  uint8_t* body;
  uint8_t* id;
  uint32_t* meta;
  uint32_t max_nodes;
  uint32_t* count;  // the caller's count word: written by the finish launch alone
};

// What the radix sort and the scan of n rows want as temporary storage (the
// larger of their needs; no device work), and the whole workspace of a call.
hipError_t shamap_temp_bytes(size_t n, size_t* bytes);
size_t shamap_workspace_bytes(size_t n, size_t temp_bytes);

// Enqueues the whole computation on `stream`; no host wait.  key / leaf (or
// null: the leaf hash is the key) n * 32 bytes, 16-byte aligned; select (or
// null: every row) ceil(n / 64) words; ws of shamap_workspace_bytes, 256-byte
// aligned.  root (32 bytes) and counts (4 words, or null) are written by the
// last launch alone.  fault (or null): asked before every HIP call; true makes
// the call fail there (stl_debug_fault_after).  clock (or null): marked before
// the first launch (0) and after the sort (1), the heads and neighbours (2),
// the levels (3) and the finish (4).  n >= 1.  emit (or null): every inner node
// is also stored there, by the emitting instantiation of the level kernel.
hipError_t launch_shamap_root(const uint8_t* key, const uint8_t* leaf, const uint64_t* select, uint32_t n,
                              uint8_t* root, uint32_t* counts, void* ws, size_t temp_bytes, bool (*fault)(),
                              const PhaseClock* clock, hipStream_t stream, const ShamapEmit* emit = nullptr);

// ---- the parts the resident tree (stl_shamap_tree.hip) runs on arrays of its own ----
// The same sort passes over n keys in a workspace of shamap_workspace_bytes(n,
// temp_bytes): perm[i] is the row at sorted position i (stable: equal keys in
// row order).  flags / idx: two arrays of n words of the workspace that are
// free once the sort is done (the root's head flags and their scan live
// there); temp: the workspace's temporary storage of temp_bytes.
struct ShamapSorted {
  const uint32_t* perm;
  uint32_t* flags;
  uint32_t* idx;
  void* temp;
};
hipError_t launch_shamap_sort(const uint8_t* key, uint32_t n, void* ws, size_t temp_bytes, bool (*fault)(),
                              hipStream_t stream, ShamapSorted* out);
// The temporary storage within a workspace of shamap_workspace_bytes(n, temp_bytes).
void* shamap_workspace_temp(size_t n, void* ws, size_t temp_bytes);
// out[i] = in[0] + .. + in[i - 1] (mod 2^32) over n words; temp of at least
// shamap_temp_bytes(n).
hipError_t shamap_exclusive_scan(void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out, size_t n,
                                 bool (*fault)(), hipStream_t stream);
// The neighbour kernel and the level kernel for depths d_first down to d_last
// over sorted distinct keys skey with their hash slots: hdr (kShamapHeaderBytes,
// zero but for hdr[kShamapHdrDistinct] = the number of keys, read on the
// device); n: a host-known bound of that number, which sizes the grids and the
// neighbour bytes l.  Afterwards the slot of the first key of every node at
// depth d_last holds that node's hash.  emit (or null): the nodes of those
// depths are stored, numbered by hdr[kShamapHdrEmitted]; emit->count is not written.
hipError_t launch_shamap_levels(uint32_t* hdr, int8_t* l, const uint8_t* skey, uint8_t* slot, uint32_t n,
                                uint32_t d_first, uint32_t d_last, bool (*fault)(), hipStream_t stream,
                                const ShamapEmit* emit = nullptr);
// The two halves of launch_shamap_levels on their own, for a caller that
// interleaves the level launches of two arrays (stl_shamap_fetch.hip): the
// neighbour kernel, once per array, and the plain level kernel for one depth.
hipError_t launch_shamap_neighbours(uint32_t* hdr, int8_t* l, const uint8_t* skey, uint32_t n, bool (*fault)(),
                                    hipStream_t stream);
hipError_t launch_shamap_level(uint32_t* hdr, const int8_t* l, const uint8_t* skey, uint8_t* slot, uint32_t n,
                               uint32_t d, bool (*fault)(), hipStream_t stream);

}  // namespace stl

// ---- host side of the node-storing calls (stl_api_shamap.cpp), shared with stl_api_shamap_tree.cpp ----
struct stl_shamap_nodes_out;
namespace stl {
struct Device;
struct HostCall;
// The argument checks of a stl_shamap_nodes_out: STL_OK or STL_EINVAL, no device work.
int check_nodes_out(const stl_shamap_nodes_out* out, bool device_form);
ShamapEmit emit_of(const stl_shamap_nodes_out& out);
// A host form's staging of the node arrays on the device (under the device's
// mutex: the device's own buffers, grown to max_nodes rows), and their way back:
// fetch waits for the count and names min(count, max_nodes) rows as the call's outputs.
struct NodeStage {
  ShamapEmit emit{};
  int ensure(Device& d, const stl_shamap_nodes_out& out);
  int fetch(HostCall& call, const stl_shamap_nodes_out& out);
};
}  // namespace stl
