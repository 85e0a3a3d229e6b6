// stl_shamap.hip -- gfx950 kernels of the SHAMap root (stl_shamap_root*): the
// hash a node compares for a transaction set, from the set's keys and leaf
// hashes alone (stl_shamap_core.h has the tree's rules).
//
//   1. sort     four stable 64-bit radix passes (rocPRIM) over (sort word,
//               row), least significant word first; with a select bitmap a
//               fifth pass of one bit puts the unselected rows last
//   2. heads    a position holds a distinct key when it is selected and its key
//               differs from the position before; an exclusive scan (rocPRIM)
//               numbers them, and the compact kernel copies key and leaf hash
//               of distinct key j to sorted position j.  Of equal keys the
//               first position stays: by the sort's stability, the lowest row.
//   3. neighbours   l_j, one byte per distinct key, and the inner nodes per depth
//   4. levels   depth 63 down to 0, one launch each on the stream; a launch
//               whose depth holds no node returns at once
//   5. finish   root and counts -- the only launch that writes the caller's
//               outputs
//
// A node's hash lives in the 32-byte slot of its first key's sorted position;
// a slot starts out as its key's leaf hash.  So the hash of branch c of the
// node at (d, a) is the slot of the first position in the node's range whose
// nibble d is c, whether that child is a leaf or the inner node the level
// below has just hashed; the node reads its 16 slots (a's own among them) and
// then writes slot a.  Nodes of one depth have disjoint ranges, and within a
// workgroup every read comes before a barrier and every write after it.
//
// The level kernel: a workgroup walks consecutive chunks of 256 positions,
// lists the nodes that start there (at most 128 per chunk: a node's first two
// keys are both in its range) until 128 are listed or its span ends, and lane
// groups of 16 gather each node's record into LDS -- a
// bounded search for the end of the range and for the branch's first
// position, one 32-byte load.  Then every lane hashes one record out of LDS:
// 129 dwords apart, an odd stride, so the lanes of a wave read 64 different
// banks.  128 records are 66,048 bytes: two workgroups fit a CU's 160 KB.
//
// The resident tree (stl_shamap_tree.hip) runs the sort passes, the scan and
// the neighbour and level kernels for a range of depths on arrays of its own
// (launch_shamap_sort, shamap_exclusive_scan, launch_shamap_levels).
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "stl_shamap.h"

#include "stl_shamap_core.h"

namespace stl {

namespace {

constexpr uint32_t kSmBlock = 256;       // 4 waves per workgroup
constexpr uint32_t kSmTileNodes = 128;   // nodes that can start within 256 positions
constexpr uint32_t kSmLevelGrid = 1024;  // the level kernel's fixed grid: spans beyond it by stride
constexpr uint32_t kSmSpansWanted = 512; // workgroups a depth is spread over before they are filled further
constexpr uint32_t kSmSpanChunksMax = 16;  // chunks of 256 positions one workgroup walks at most per span
// header words (kShamapHeaderBytes)
constexpr uint32_t kHdrDistinct = kShamapHdrDistinct, kHdrSelected = 65;

__device__ __forceinline__ void sm_st8(uint8_t* p, size_t row, const uint32_t k[8]) {
  uint4* q = reinterpret_cast<uint4*>(p + 32 * row);
  q[0] = make_uint4(k[0], k[1], k[2], k[3]);
  q[1] = make_uint4(k[4], k[5], k[6], k[7]);
}

__device__ __forceinline__ bool sm_selected(const uint64_t* __restrict__ select, uint32_t row) {
  return !select || ((select[row >> 6] >> (row & 63u)) & 1ull);
}

// Sort word w of the key at position i: of row perm[i], or of row i (the first
// pass, which also writes the identity into vout).
__global__ __launch_bounds__(kSmBlock) void shamap_sort_word_kernel(const uint8_t* __restrict__ key,
                                                                    const uint32_t* __restrict__ perm, uint32_t n,
                                                                    uint32_t w, uint64_t* __restrict__ kout,
                                                                    uint32_t* __restrict__ vout) {
  const uint32_t i = blockIdx.x * kSmBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t row = perm ? perm[i] : i;
  const uint2 v = *reinterpret_cast<const uint2*>(key + 32 * (size_t)row + 8 * w);
  kout[i] = be64_from_le32(v.x, v.y);
  if (!perm) vout[i] = i;
}

// The last pass's key: 0 for a selected row, 1 for the others.
__global__ __launch_bounds__(kSmBlock) void shamap_select_word_kernel(const uint64_t* __restrict__ select,
                                                                      const uint32_t* __restrict__ perm, uint32_t n,
                                                                      uint32_t* __restrict__ kout) {
  const uint32_t i = blockIdx.x * kSmBlock + threadIdx.x;
  if (i >= n) return;
  kout[i] = sm_selected(select, perm[i]) ? 0u : 1u;
}

// flags[i] = position i holds a distinct key; hdr[kHdrSelected] += the selected positions.
__global__ __launch_bounds__(kSmBlock) void shamap_head_kernel(const uint8_t* __restrict__ key,
                                                               const uint64_t* __restrict__ select,
                                                               const uint32_t* __restrict__ perm, uint32_t n,
                                                               uint32_t* __restrict__ flags,
                                                               uint32_t* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * kSmBlock + threadIdx.x;
  bool sel = false, head = false;
  if (i < n) {
    const uint32_t row = perm[i];
    sel = sm_selected(select, row);
    head = sel;
    if (sel && i > 0) {
      // the selected rows come first, so the position before is selected too
      uint32_t a[8], b[8];
      shamap_load_key(a, key, row);
      shamap_load_key(b, key, perm[i - 1]);
      head = shamap_common_prefix(a, b) < 64u;
    }
    flags[i] = head ? 1u : 0u;
  }
  const uint64_t sw = __ballot(sel);
  if ((threadIdx.x & 63u) == 0 && sw != 0) atomicAdd(&hdr[kHdrSelected], (uint32_t)__popcll(sw));
}

// Distinct key j (flags, idx: its number) -> skey[j], slot[j]; the last
// position writes the number of distinct keys.
__global__ __launch_bounds__(kSmBlock) void shamap_compact_kernel(const uint8_t* __restrict__ key,
                                                                  const uint8_t* __restrict__ leaf,
                                                                  const uint32_t* __restrict__ perm,
                                                                  const uint32_t* __restrict__ flags,
                                                                  const uint32_t* __restrict__ idx, uint32_t n,
                                                                  uint8_t* __restrict__ skey,
                                                                  uint8_t* __restrict__ slot,
                                                                  uint32_t* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * kSmBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t f = flags[i], j = idx[i];
  if (i == n - 1) hdr[kHdrDistinct] = j + f;
  if (!f) return;
  const uint32_t row = perm[i];
  uint32_t k[8];
  shamap_load_key(k, key, row);
  sm_st8(skey, j, k);
  if (leaf) shamap_load_key(k, leaf, row);
  sm_st8(slot, j, k);
}

// l[j] for every distinct key, and hdr[d] += the inner nodes that start at depth d.
__global__ __launch_bounds__(kSmBlock) void shamap_neighbour_kernel(const uint8_t* __restrict__ skey, uint32_t n,
                                                                    int8_t* __restrict__ l,
                                                                    uint32_t* __restrict__ hdr) {
  __shared__ uint32_t hist[kShamapDepths];
  if (threadIdx.x < kShamapDepths) hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t m = hdr[kHdrDistinct];
  const uint32_t j = blockIdx.x * kSmBlock + threadIdx.x;
  if (j < m && j < n) {
    uint32_t a[8], b[8];
    shamap_load_key(a, skey, j);
    int32_t lp = -1;
    if (j > 0) {
      shamap_load_key(b, skey, j - 1);
      lp = (int32_t)shamap_common_prefix(b, a);
    }
    const bool last = j + 1 == m;
    if (!last) shamap_load_key(b, skey, j + 1);
    const int32_t lc = shamap_neighbour(a, b, last, m == 1);
    l[j] = (int8_t)lc;
    for (int32_t d = lp + 1; d <= lc; ++d) atomicAdd(&hist[d], 1u);
  }
  __syncthreads();
  if (threadIdx.x < kShamapDepths && hist[threadIdx.x]) atomicAdd(&hdr[threadIdx.x], hist[threadIdx.x]);
}

// What the emitting level kernel is given: ShamapEmit's arrays and the header
// word the rows are numbered from (never one the kernel reads through hdr).
struct SmEmit {
  uint8_t* hash;
  uint8_t* body;
  uint8_t* id;
  uint32_t* meta;
  uint32_t max_nodes;
  uint32_t* counter;
};

// Gathers and hashes the `count` nodes listed in node_pos (the whole workgroup).
// kEmit: the nodes are also stored (ShamapEmit): the tile takes `count` row
// numbers from the call's counter word with one add, the gather lanes note which
// branches are leaves, and after the hash the tile goes out -- the bodies
// straight from the LDS records, 16 bytes per lane, consecutive lanes on
// consecutive pieces of a row, so a wave writes whole 128-byte lines.  Every
// store is guarded by the row number being below max_nodes.
template <bool kEmit>
__device__ __forceinline__ void shamap_flush(uint32_t* rec, const uint32_t* node_pos, uint32_t count, uint32_t m,
                                             const uint8_t* __restrict__ skey, uint8_t* slot, uint32_t d,
                                             const int8_t* __restrict__ l, const SmEmit& em, uint32_t* node_leaf,
                                             uint32_t* tile_base) {
  const uint32_t tid = threadIdx.x;
  __syncthreads();  // node_pos is written
  if constexpr (kEmit) {
    if (tid == 0) *tile_base = atomicAdd(em.counter, count);
  }
  // gather: 16 lanes per node, one per branch
  const uint32_t c = tid & 15u;
  for (uint32_t k = tid >> 4; k < count; k += kSmBlock / 16) {
    const uint32_t a = node_pos[k];
    const uint32_t e = shamap_range_end(skey, m, a, d);
    const uint32_t p = shamap_branch_first(skey, a, e, d, c);
    uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0;
    if (p < e) {
      const uint4* q = reinterpret_cast<const uint4*>(slot + 32 * (size_t)p);
      h0 = q[0];
      h1 = q[1];
    }
    if constexpr (kEmit) {
      // the 16 lanes of a node sit side by side in their wave and leave the loop together
      const uint64_t leaves = __ballot(p < e && shamap_branch_is_leaf(l, p, e, d));
      if (c == 0) node_leaf[k] = (uint32_t)(leaves >> (tid & 48u)) & 0xffffu;
    }
    uint32_t* r = rec + k * kShamapRecordWords;
    if (c == 0) r[0] = kShamapInnerPrefix;
    r += 1 + 8 * c;
    r[0] = h0.x; r[1] = h0.y; r[2] = h0.z; r[3] = h0.w;
    r[4] = h1.x; r[5] = h1.y; r[6] = h1.z; r[7] = h1.w;
  }
  __syncthreads();  // every slot this workgroup reads has been read
  // hash: one lane per record
  if (tid < count) {
    uint32_t out[8];
    shamap_inner_hash(out, rec + tid * kShamapRecordWords);
    const uint32_t a = node_pos[tid];
    sm_st8(slot, a, out);
    if constexpr (kEmit) {
      const uint32_t row = *tile_base + tid;
      if (row < em.max_nodes) {
        sm_st8(em.hash, row, out);
        if (em.id) {
          uint32_t key[8], id[8];
          shamap_load_key(key, skey, a);
          shamap_mask_key(id, key, d);
          sm_st8(em.id, row, id);
        }
        if (em.meta) em.meta[row] = shamap_node_meta(d, node_leaf[tid]);
      }
    }
  }
  if constexpr (kEmit) {
    // the bodies: piece q is 16 bytes, 32 pieces to a row
    const uint32_t base = *tile_base;
    for (uint32_t q = tid; q < 32u * count; q += kSmBlock) {
      const uint32_t k = q >> 5, part = q & 31u;
      if (base + k >= em.max_nodes) continue;
      const uint32_t* r = rec + k * kShamapRecordWords + 1 + 4 * part;
      *reinterpret_cast<uint4*>(em.body + 512 * (size_t)(base + k) + 16 * part) = make_uint4(r[0], r[1], r[2], r[3]);
    }
  }
  __syncthreads();  // rec and node_pos may be reused
}

// The inner nodes of depth d (see the top of the file).  A workgroup takes a
// span of consecutive 256-position chunks and collects the nodes that start in
// them until the next chunk's would not fit the 128 records; then it gathers
// and hashes those together.  The span is sized from the depth's node count so
// that a sparse depth (a few nodes per thousand positions: clustered keys)
// still fills the hashing lanes, while at least kSmSpansWanted workgroups
// share the depth.
template <bool kEmit>
__global__ __launch_bounds__(kSmBlock) void shamap_level_kernel(const uint32_t* __restrict__ hdr,
                                                                const int8_t* __restrict__ l,
                                                                const uint8_t* __restrict__ skey, uint8_t* slot,
                                                                uint32_t d, SmEmit em) {
  __shared__ uint32_t rec[kSmTileNodes * kShamapRecordWords];
  __shared__ uint32_t node_pos[kSmTileNodes];
  __shared__ uint32_t wave_nodes[kSmBlock / 64];
  __shared__ uint32_t node_leaf[kEmit ? kSmTileNodes : 1];
  __shared__ uint32_t tile_base[1];
  const uint32_t nodes = hdr[d];
  if (nodes == 0) return;  // uniform: no node at this depth
  const uint32_t m = hdr[kHdrDistinct];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t chunks = (m + kSmBlock - 1) / kSmBlock;
  // nodes a workgroup should meet, and the chunks that hold about that many
  uint32_t want = (nodes + kSmSpansWanted - 1) / kSmSpansWanted;
  if (want > kSmTileNodes) want = kSmTileNodes;
  uint32_t per = (uint32_t)(((uint64_t)chunks * want) / nodes);
  if (per == 0) per = 1;
  if (per > kSmSpanChunksMax) per = kSmSpanChunksMax;  // a depth of a few nodes is still scanned side by side
  const uint32_t spans = (chunks + per - 1) / per;
  for (uint32_t span = blockIdx.x; span < spans; span += gridDim.x) {
    const uint32_t first = span * per, past = first + per < chunks ? first + per : chunks;
    uint32_t count = 0;  // uniform: nodes listed and not yet hashed
    for (uint32_t ch = first; ch < past; ++ch) {
      const uint32_t i = ch * kSmBlock + tid;
      bool starts = false;
      if (i < m) starts = shamap_starts_node(i ? (int32_t)l[i - 1] : -1, (int32_t)l[i], (int32_t)d);
      const uint64_t sw = __ballot(starts);
      if (lane == 0) wave_nodes[wave] = (uint32_t)__popcll(sw);
      __syncthreads();
      uint32_t base = 0, here = 0;  // here <= 128: two starts are never adjacent
#pragma unroll
      for (uint32_t v = 0; v < kSmBlock / 64; ++v) {
        if (v < wave) base += wave_nodes[v];
        here += wave_nodes[v];
      }
      if (count + here > kSmTileNodes) {  // uniform
        shamap_flush<kEmit>(rec, node_pos, count, m, skey, slot, d, l, em, node_leaf, tile_base);
        count = 0;
      }
      if (starts) {
        const uint32_t k = count + base + (uint32_t)__popcll(sw & ((1ull << lane) - 1ull));
        if (k < kSmTileNodes) node_pos[k] = i;  // always
      }
      count += here;
      if (count > kSmTileNodes) count = kSmTileNodes;  // never
      __syncthreads();  // wave_nodes is reused by the next chunk
    }
    if (count) shamap_flush<kEmit>(rec, node_pos, count, m, skey, slot, d, l, em, node_leaf, tile_base);
  }
}

// root = slot 0 (zeros for the empty map); counts; the number of stored nodes (or null).
__global__ __launch_bounds__(64) void shamap_finish_kernel(const uint32_t* __restrict__ hdr,
                                                           const uint8_t* __restrict__ slot,
                                                           uint32_t* __restrict__ root,
                                                           uint32_t* __restrict__ counts,
                                                           uint32_t* __restrict__ emitted) {
  const uint32_t t = threadIdx.x;
  const uint32_t m = hdr[kHdrDistinct];
  if (t == 0 && emitted) *emitted = hdr[kShamapHdrEmitted];
  if (t < 8) root[t] = m ? reinterpret_cast<const uint32_t*>(slot)[t] : 0u;
  const uint32_t nodes = hdr[t];
  // the sum over the depths and the deepest depth in use, by wave reduction
  uint32_t sum = nodes, deep = nodes ? t : 0u;
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_xor(sum, off);
    const uint32_t o = __shfl_xor(deep, off);
    deep = o > deep ? o : deep;
  }
  if (t == 0 && counts) {
    counts[0] = m;
    counts[1] = hdr[kHdrSelected] - m;
    counts[2] = sum;
    counts[3] = deep;
  }
}

uint32_t grid_of(uint32_t n) { return (n + kSmBlock - 1) / kSmBlock; }

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// The workspace's parts, in order.
struct ShamapWs {
  uint32_t* hdr;
  uint64_t* k[2];
  uint32_t* v[2];
  int8_t* l;
  uint8_t* skey;
  uint8_t* slot;
  void* temp;
  size_t bytes;
  ShamapWs(void* ws, size_t n, size_t temp_bytes) {
    uint8_t* p = static_cast<uint8_t*>(ws);
    size_t o = 0;
    auto take = [&](size_t b) {
      uint8_t* q = p + o;
      o += up256(b);
      return q;
    };
    hdr = reinterpret_cast<uint32_t*>(take(kShamapHeaderBytes));
    k[0] = reinterpret_cast<uint64_t*>(take(8 * n));
    k[1] = reinterpret_cast<uint64_t*>(take(8 * n));
    v[0] = reinterpret_cast<uint32_t*>(take(4 * n));
    v[1] = reinterpret_cast<uint32_t*>(take(4 * n));
    l = reinterpret_cast<int8_t*>(take(n));
    skey = take(32 * n);
    slot = take(32 * n);
    temp = take(temp_bytes);
    bytes = o;
  }
};

}  // namespace

hipError_t shamap_temp_bytes(size_t n, size_t* bytes) {
  *bytes = 0;
  if (n == 0) return hipSuccess;
  size_t a = 0, b = 0, c = 0;
  rocprim::double_buffer<uint64_t> k64(nullptr, nullptr);
  rocprim::double_buffer<uint32_t> k32(nullptr, nullptr), v(nullptr, nullptr);
  hipError_t e = rocprim::radix_sort_pairs(nullptr, a, k64, v, n, 0, 64, nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::radix_sort_pairs(nullptr, b, k32, v, n, 0, 1, nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(nullptr, c, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), 0u, n,
                              rocprim::plus<uint32_t>(), nullptr);
  if (e != hipSuccess) return e;
  *bytes = a > b ? (a > c ? a : c) : (b > c ? b : c);
  return hipSuccess;
}

size_t shamap_workspace_bytes(size_t n, size_t temp_bytes) { return ShamapWs(nullptr, n, temp_bytes).bytes; }

#define SM_TRY(expr)                             \
  do {                                           \
    if (fault && fault()) return hipErrorUnknown; \
    const hipError_t e_ = (expr);                \
    if (e_ != hipSuccess) return e_;             \
  } while (0)

#define SM_LAUNCH(kernel, grid, block, ...)                             \
  do {                                                                  \
    if (fault && fault()) return hipErrorUnknown;                       \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
    const hipError_t e_ = hipGetLastError();                            \
    if (e_ != hipSuccess) return e_;                                    \
  } while (0)

static bool shamap_emit_ok(const ShamapEmit& e) {
  return e.hash && e.body && !(((uintptr_t)e.hash | (uintptr_t)e.body | (uintptr_t)e.id) & 15u) &&
         !((uintptr_t)e.meta & 3u);
}

// The level kernel for depths d_first down to d_last, one launch each: the
// emitting instantiation when the nodes are stored, else the plain one.
static hipError_t shamap_level_launches(uint32_t* hdr, const int8_t* l, const uint8_t* skey, uint8_t* slot,
                                        uint32_t grid, uint32_t d_first, uint32_t d_last, const ShamapEmit* emit,
                                        bool (*fault)(), hipStream_t stream) {
  SmEmit em{};
  if (emit) em = SmEmit{emit->hash, emit->body, emit->id, emit->meta, emit->max_nodes, hdr + kShamapHdrEmitted};
  for (int d = (int)d_first; d >= (int)d_last; --d) {
    if (emit)
      SM_LAUNCH(shamap_level_kernel<true>, grid, kSmBlock, hdr, l, skey, slot, (uint32_t)d, em);
    else
      SM_LAUNCH(shamap_level_kernel<false>, grid, kSmBlock, hdr, l, skey, slot, (uint32_t)d, em);
  }
  return hipSuccess;
}

// The four stable radix passes over (sort word, row), least significant word first.
static hipError_t shamap_sort_passes(const uint8_t* key, uint32_t n, const ShamapWs& w, size_t temp_bytes,
                                     rocprim::double_buffer<uint64_t>& k64, rocprim::double_buffer<uint32_t>& v,
                                     bool (*fault)(), hipStream_t stream) {
  const uint32_t g = grid_of(n);
  for (int word = 3; word >= 0; --word) {
    SM_LAUNCH(shamap_sort_word_kernel, g, kSmBlock, key, word == 3 ? nullptr : v.current(), n, (uint32_t)word,
              k64.current(), v.current());
    size_t tb = temp_bytes;
    SM_TRY(rocprim::radix_sort_pairs(w.temp, tb, k64, v, n, 0, 64, stream));
  }
  return hipSuccess;
}

hipError_t launch_shamap_root(const uint8_t* key, const uint8_t* leaf, const uint64_t* select, uint32_t n,
                              uint8_t* root, uint32_t* counts, void* ws, size_t temp_bytes, bool (*fault)(),
                              const PhaseClock* clock, hipStream_t stream, const ShamapEmit* emit) {
  if (n == 0 || !key || !root || !ws) return hipErrorInvalidValue;
  if (emit && !shamap_emit_ok(*emit)) return hipErrorInvalidValue;
  if (((uintptr_t)key & 15u) || ((uintptr_t)leaf & 15u) || ((uintptr_t)root & 3u) || ((uintptr_t)ws & 255u))
    return hipErrorInvalidValue;
  const ShamapWs w(ws, n, temp_bytes);
  const uint32_t g = grid_of(n);
  if (clock) clock->mark(clock->ctx, stream, 0);
  SM_TRY(hipMemsetAsync(w.hdr, 0, kShamapHeaderBytes, stream));
  // 1. sort
  rocprim::double_buffer<uint64_t> k64(w.k[0], w.k[1]);
  rocprim::double_buffer<uint32_t> v(w.v[0], w.v[1]);
  {
    const hipError_t e = shamap_sort_passes(key, n, w, temp_bytes, k64, v, fault, stream);
    if (e != hipSuccess) return e;
  }
  if (select) {
    rocprim::double_buffer<uint32_t> k32(reinterpret_cast<uint32_t*>(w.k[0]), reinterpret_cast<uint32_t*>(w.k[1]));
    SM_LAUNCH(shamap_select_word_kernel, g, kSmBlock, select, v.current(), n, k32.current());
    size_t tb = temp_bytes;
    SM_TRY(rocprim::radix_sort_pairs(w.temp, tb, k32, v, n, 0, 1, stream));
  }
  if (clock) clock->mark(clock->ctx, stream, 1);
  // 2. heads, 3. neighbours
  uint32_t* flags = reinterpret_cast<uint32_t*>(w.k[0]);
  uint32_t* idx = reinterpret_cast<uint32_t*>(w.k[1]);
  SM_LAUNCH(shamap_head_kernel, g, kSmBlock, key, select, v.current(), n, flags, w.hdr);
  {
    size_t tb = temp_bytes;
    SM_TRY(rocprim::exclusive_scan(w.temp, tb, flags, idx, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream));
  }
  SM_LAUNCH(shamap_compact_kernel, g, kSmBlock, key, leaf, v.current(), flags, idx, n, w.skey, w.slot, w.hdr);
  SM_LAUNCH(shamap_neighbour_kernel, g, kSmBlock, w.skey, n, w.l, w.hdr);
  if (clock) clock->mark(clock->ctx, stream, 2);
  // 4. levels
  const uint32_t lg = g < kSmLevelGrid ? g : kSmLevelGrid;
  {
    const hipError_t e = shamap_level_launches(w.hdr, w.l, w.skey, w.slot, lg, kShamapDepths - 1, 0, emit, fault, stream);
    if (e != hipSuccess) return e;
  }
  if (clock) clock->mark(clock->ctx, stream, 3);
  // 5. finish
  SM_LAUNCH(shamap_finish_kernel, 1, 64, w.hdr, w.slot, reinterpret_cast<uint32_t*>(root), counts,
            emit ? emit->count : static_cast<uint32_t*>(nullptr));
  if (clock) clock->mark(clock->ctx, stream, 4);
  return hipSuccess;
}

hipError_t launch_shamap_sort(const uint8_t* key, uint32_t n, void* ws, size_t temp_bytes, bool (*fault)(),
                              hipStream_t stream, ShamapSorted* out) {
  if (n == 0 || !key || !ws || !out || ((uintptr_t)key & 15u) || ((uintptr_t)ws & 255u)) return hipErrorInvalidValue;
  const ShamapWs w(ws, n, temp_bytes);
  rocprim::double_buffer<uint64_t> k64(w.k[0], w.k[1]);
  rocprim::double_buffer<uint32_t> v(w.v[0], w.v[1]);
  const hipError_t e = shamap_sort_passes(key, n, w, temp_bytes, k64, v, fault, stream);
  if (e != hipSuccess) return e;
  out->perm = v.current();
  out->flags = reinterpret_cast<uint32_t*>(w.k[0]);
  out->idx = reinterpret_cast<uint32_t*>(w.k[1]);
  out->temp = w.temp;
  return hipSuccess;
}

void* shamap_workspace_temp(size_t n, void* ws, size_t temp_bytes) { return ShamapWs(ws, n, temp_bytes).temp; }

hipError_t shamap_exclusive_scan(void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out, size_t n,
                                 bool (*fault)(), hipStream_t stream) {
  size_t tb = temp_bytes;
  SM_TRY(rocprim::exclusive_scan(temp, tb, in, out, 0u, n, rocprim::plus<uint32_t>(), stream));
  return hipSuccess;
}

hipError_t launch_shamap_levels(uint32_t* hdr, int8_t* l, const uint8_t* skey, uint8_t* slot, uint32_t n,
                                uint32_t d_first, uint32_t d_last, bool (*fault)(), hipStream_t stream,
                                const ShamapEmit* emit) {
  if (n == 0 || !hdr || !l || !skey || !slot || d_first >= kShamapDepths || d_last > d_first)
    return hipErrorInvalidValue;
  if (emit && !shamap_emit_ok(*emit)) return hipErrorInvalidValue;
  const uint32_t g = grid_of(n);
  SM_LAUNCH(shamap_neighbour_kernel, g, kSmBlock, skey, n, l, hdr);
  const uint32_t lg = g < kSmLevelGrid ? g : kSmLevelGrid;
  return shamap_level_launches(hdr, l, skey, slot, lg, d_first, d_last, emit, fault, stream);
}

hipError_t launch_shamap_neighbours(uint32_t* hdr, int8_t* l, const uint8_t* skey, uint32_t n, bool (*fault)(),
                                    hipStream_t stream) {
  if (n == 0 || !hdr || !l || !skey) return hipErrorInvalidValue;
  SM_LAUNCH(shamap_neighbour_kernel, grid_of(n), kSmBlock, skey, n, l, hdr);
  return hipSuccess;
}

hipError_t launch_shamap_level(uint32_t* hdr, const int8_t* l, const uint8_t* skey, uint8_t* slot, uint32_t n,
                               uint32_t d, bool (*fault)(), hipStream_t stream) {
  if (n == 0 || !hdr || !l || !skey || !slot || d >= kShamapDepths) return hipErrorInvalidValue;
  const uint32_t g = grid_of(n);
  return shamap_level_launches(hdr, l, skey, slot, g < kSmLevelGrid ? g : kSmLevelGrid, d, d, nullptr, fault, stream);
}

}  // namespace stl
