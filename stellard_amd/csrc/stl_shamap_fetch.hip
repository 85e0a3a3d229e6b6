// stl_shamap_fetch.hip -- gfx950 kernels of the fetch pack between two resident
// SHAMaps (stl_shamap_tree_fetch_pack*; stl_shamap_fetch_core.h has the rules).
// Nothing here writes a tree: every array written is the stream context's.
//
// One call, all on the caller's stream:
//   1. buckets   65,536 lanes compare the two live generations' bucket values; a
//                bucket that differs sends want's keys to want's scratch when they
//                make an inner node, and have's to have's when both do; the two
//                count arrays and the two row counts are scanned
//   2. gather    one lane per scratch row copies key and leaf hash, in order;
//                the neighbour kernel of stl_shamap.hip runs over each scratch
//   3. levels    depth 63 down to 4: the plain level kernel over have's scratch,
//                then fetch_level_kernel over want's -- the level kernel's
//                listing, gather and hash, and after the hash every node asks
//                have's scratch for an inner node at its ID (a bisection; that
//                node's hash is in the slot of its first key exactly now).  Only
//                nodes have does not hold take row numbers: the keep flags are
//                counted per wave by ballot, the tile takes its rows with one
//                add, and the bodies go out of the LDS records by a per-node row.
//   4. top       four launches fold both trees' bucket values into the 4,369
//                prefixes above them, side by side, and store want's where have's
//                is no inner node or hashes differently
//   5. finish    the count and the eight counts -- the only launch that writes
//                the caller's count words
//
// Every count is read on the device; the grids come from the hosts' bounds of the
// two item counts.  Every read of a generation is clamped by its count and
// capacity, every store into a scratch by the rows it was sized for, every store
// into the caller's arrays by max_nodes.
#include "stl_shamap_fetch.h"

#include "stl_shamap.h"
#include "stl_shamap_fetch_core.h"

namespace stl {

namespace {

constexpr uint32_t kFpBlock = 256;      // 4 waves per workgroup
constexpr uint32_t kFpTileNodes = 128;  // as stl_shamap.hip's level kernel: nodes that can start within 256 positions
constexpr uint32_t kFpLevelGrid = 1024;
constexpr uint32_t kFpSpansWanted = 512;
constexpr uint32_t kFpSpanChunksMax = 16;
constexpr uint32_t kFpNoRow = 0xffffffffu;  // above every max_nodes
// header words of the workspace
constexpr uint32_t kFhEmitted = 0, kFhBuckets = 1, kFhCandidates = 2, kFhSuppressed = 3, kFhWords = 64;
// a tree's top values: the prefixes of length 3, 2, 1 and the root, one after another
constexpr uint32_t kFpTopValues = kTreeTopValues + 1;

__device__ __forceinline__ void fp_st8(uint8_t* p, size_t row, const uint32_t k[8]) {
  uint4* q = reinterpret_cast<uint4*>(p + 32 * row);
  q[0] = make_uint4(k[0], k[1], k[2], k[3]);
  q[1] = make_uint4(k[4], k[5], k[6], k[7]);
}

__device__ __forceinline__ void fp_count(bool v, uint32_t* word) {
  const uint64_t b = __ballot(v);
  if ((threadIdx.x & 63u) == 0 && b != 0) atomicAdd(word, (uint32_t)__popcll(b));
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
uint32_t grid_of(uint32_t n) { return (n + kFpBlock - 1) / kFpBlock; }

// One side's scratch: what launch_shamap_levels works on.
struct FetchScratch {
  uint32_t* hdr;
  int8_t* l;
  uint8_t *skey, *slot;
};

// The workspace's parts, in order.  The header and the two scratch headers lie
// side by side: one memset clears them.
struct FetchWs {
  uint32_t *fh, *begin_w, *begin_h, *sz_w, *off_w, *sz_h, *off_h, *topcnt_w, *toph_w, *topcnt_h, *toph_h;
  FetchScratch w, h;
  void* temp;
  size_t bytes;
  FetchWs(void* base, size_t want_rows, size_t have_rows, size_t temp_bytes) {
    uint8_t* p = static_cast<uint8_t*>(base);
    size_t o = 0;
    auto take = [&](size_t b) {
      uint8_t* q = p + o;
      o += up256(b);
      return q;
    };
    auto words = [&](size_t n) { return reinterpret_cast<uint32_t*>(take(4 * n)); };
    fh = words(kFhWords);
    w.hdr = reinterpret_cast<uint32_t*>(take(kShamapHeaderBytes));
    h.hdr = reinterpret_cast<uint32_t*>(take(kShamapHeaderBytes));
    begin_w = words(kTreeBuckets);
    begin_h = words(kTreeBuckets);
    sz_w = words(kTreeBuckets);
    off_w = words(kTreeBuckets);
    sz_h = words(kTreeBuckets);
    off_h = words(kTreeBuckets);
    topcnt_w = words(kFpTopValues);
    toph_w = words(8 * kFpTopValues);
    topcnt_h = words(kFpTopValues);
    toph_h = words(8 * kFpTopValues);
    w.l = reinterpret_cast<int8_t*>(take(want_rows));
    w.skey = take(32 * want_rows);
    w.slot = take(32 * want_rows);
    h.l = reinterpret_cast<int8_t*>(take(have_rows));
    h.skey = take(32 * have_rows);
    h.slot = take(32 * have_rows);
    temp = p + o;
    bytes = o + up256(temp_bytes);
  }
  size_t cleared() const { return 4 * kFhWords + 2 * kShamapHeaderBytes; }
};

// 1. kTreeBuckets lanes exactly.  have_cnt null: no tree -- every bucket of it is empty.
__global__ __launch_bounds__(kFpBlock) void fetch_buckets_kernel(const uint32_t* __restrict__ want_cnt,
                                                                 const uint32_t* __restrict__ want_h,
                                                                 const uint32_t* __restrict__ have_cnt,
                                                                 const uint32_t* __restrict__ have_h,
                                                                 uint32_t* __restrict__ sz_w,
                                                                 uint32_t* __restrict__ sz_h, uint32_t* fh) {
  const uint32_t b = blockIdx.x * kFpBlock + threadIdx.x;
  uint32_t x[8], y[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  shamap_load_key(x, reinterpret_cast<const uint8_t*>(want_h), b);
  const uint32_t cw = want_cnt[b];
  uint32_t ch = 0;
  if (have_cnt) {
    ch = have_cnt[b];
    shamap_load_key(y, reinterpret_cast<const uint8_t*>(have_h), b);
  }
  const bool differs = shamap_bucket_differs(cw, x, ch, y);
  sz_w[b] = shamap_fetch_want_rows(differs, cw);
  sz_h[b] = shamap_fetch_have_rows(differs, cw, ch);
  fp_count(differs, &fh[kFhBuckets]);
}

// 2. scratch row p <- the row of its bucket in generation g (count m, clamped by
// cap).  rows: what the scratch was sized for.  The first lane states the total.
__global__ __launch_bounds__(kFpBlock) void fetch_gather_kernel(const uint8_t* __restrict__ gkey,
                                                                const uint8_t* __restrict__ gleaf,
                                                                const uint32_t* __restrict__ gcnt,
                                                                const uint32_t* __restrict__ meta, uint32_t cap,
                                                                const uint32_t* __restrict__ begin,
                                                                const uint32_t* __restrict__ sz,
                                                                const uint32_t* __restrict__ off, uint32_t rows,
                                                                uint32_t* __restrict__ hdr, uint8_t* __restrict__ skey,
                                                                uint8_t* __restrict__ slot) {
  const uint32_t p = blockIdx.x * kFpBlock + threadIdx.x;
  uint32_t total = off[kTreeBuckets - 1] + sz[kTreeBuckets - 1];
  if (total > rows) total = rows;  // never: no more keys are gathered than the tree holds
  if (p == 0) hdr[kShamapHdrDistinct] = total;
  if (p >= total) return;
  const uint32_t m = shamap_tree_readable(meta[0], cap);
  const uint32_t b = shamap_diff_bucket_of(off, p);
  uint32_t lo, hi;
  shamap_lookup_range(begin[b], gcnt[b], m, &lo, &hi);
  const uint32_t src = lo + (p - off[b]);
  uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (src < hi) shamap_load_key(v, gkey, src);  // always, while the counts describe the keys
  fp_st8(skey, p, v);
  if (src < hi) shamap_load_key(v, gleaf, src);
  fp_st8(slot, p, v);
}

// Where the kept nodes go (ShamapEmit's arrays) and the words that count them.
struct FetchEmit {
  uint8_t* hash;
  uint8_t* body;
  uint8_t* id;
  uint32_t* meta;
  uint32_t max_nodes;
  uint32_t* fh;
};

// 3. Gathers and hashes the `count` nodes listed in node_pos (the whole
// workgroup), as shamap_flush of stl_shamap.hip does; then every node asks have
// (hv.hdr null: no tree) whether it holds the same node, and the ones it does not
// hold are stored.  Every node's hash goes into its own slot: its parent needs it.
__device__ __forceinline__ void fetch_flush(uint32_t* rec, const uint32_t* node_pos, uint32_t count, uint32_t m,
                                            const uint8_t* __restrict__ skey, uint8_t* slot, uint32_t d,
                                            const int8_t* __restrict__ l, const FetchScratch& hv, const FetchEmit& em,
                                            uint32_t* node_leaf, uint32_t* node_row, uint32_t* wave_keep,
                                            uint32_t* tile_base) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  __syncthreads();  // node_pos is written
  // gather: 16 lanes per node, one per branch
  const uint32_t c = tid & 15u;
  for (uint32_t k = tid >> 4; k < count; k += kFpBlock / 16) {
    const uint32_t a = node_pos[k];
    const uint32_t e = shamap_range_end(skey, m, a, d);
    const uint32_t p = shamap_branch_first(skey, a, e, d, c);
    uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0;
    if (p < e) {
      const uint4* q = reinterpret_cast<const uint4*>(slot + 32 * (size_t)p);
      h0 = q[0];
      h1 = q[1];
    }
    // the 16 lanes of a node sit side by side in their wave and leave the loop together
    const uint64_t leaves = __ballot(p < e && shamap_branch_is_leaf(l, p, e, d));
    if (c == 0) node_leaf[k] = (uint32_t)(leaves >> (tid & 48u)) & 0xffffu;
    uint32_t* r = rec + k * kShamapRecordWords;
    if (c == 0) r[0] = kShamapInnerPrefix;
    r += 1 + 8 * c;
    r[0] = h0.x; r[1] = h0.y; r[2] = h0.z; r[3] = h0.w;
    r[4] = h1.x; r[5] = h1.y; r[6] = h1.z; r[7] = h1.w;
  }
  __syncthreads();  // every slot this workgroup reads has been read
  // hash and ask: one lane per record
  uint32_t out[8], id[8];
  bool keep = false;
  if (tid < count) {
    shamap_inner_hash(out, rec + tid * kShamapRecordWords);
    const uint32_t a = node_pos[tid];
    fp_st8(slot, a, out);
    uint32_t key[8];
    shamap_load_key(key, skey, a);
    shamap_mask_key(id, key, d);
    const uint32_t mh = hv.hdr ? hv.hdr[kShamapHdrDistinct] : 0u;
    keep = !shamap_fetch_have_holds(hv.skey, hv.l, hv.slot, mh, id, d, out);
  }
  const uint64_t kb = __ballot(keep);
  if (lane == 0) wave_keep[wave] = (uint32_t)__popcll(kb);
  __syncthreads();
  if (tid == 0) {
    uint32_t kept = 0;
#pragma unroll
    for (uint32_t v = 0; v < kFpBlock / 64; ++v) kept += wave_keep[v];
    *tile_base = kept ? atomicAdd(&em.fh[kFhEmitted], kept) : 0u;
    atomicAdd(&em.fh[kFhCandidates], count);
    if (count != kept) atomicAdd(&em.fh[kFhSuppressed], count - kept);
  }
  __syncthreads();  // tile_base is written
  if (tid < count) {
    uint32_t row = kFpNoRow;
    if (keep) {
      row = *tile_base + (uint32_t)__popcll(kb & ((1ull << lane) - 1ull));
#pragma unroll
      for (uint32_t v = 0; v < kFpBlock / 64; ++v)
        if (v < wave) row += wave_keep[v];
      if (row < em.max_nodes) {
        fp_st8(em.hash, row, out);
        if (em.id) fp_st8(em.id, row, id);
        if (em.meta) em.meta[row] = shamap_node_meta(d, node_leaf[tid]);
      }
    }
    node_row[tid] = row;
  }
  __syncthreads();  // node_row is written
  // the bodies of the kept nodes: piece q is 16 bytes, 32 pieces to a row, so a
  // wave's 64 lanes write two whole rows, 128-byte lines throughout
  for (uint32_t q = tid; q < 32u * count; q += kFpBlock) {
    const uint32_t k = q >> 5, part = q & 31u;
    const uint32_t row = node_row[k];
    if (row >= em.max_nodes) continue;  // suppressed (kFpNoRow), or past the caller's room
    const uint32_t* r = rec + k * kShamapRecordWords + 1 + 4 * part;
    *reinterpret_cast<uint4*>(em.body + 512 * (size_t)row + 16 * part) = make_uint4(r[0], r[1], r[2], r[3]);
  }
  __syncthreads();  // rec, node_pos, node_row and wave_keep may be reused
}

// The inner nodes of want's scratch at depth d: the listing of
// shamap_level_kernel (spans of 256-position chunks, up to 128 nodes a tile),
// flushed by fetch_flush.
__global__ __launch_bounds__(kFpBlock) void fetch_level_kernel(const uint32_t* __restrict__ hdr,
                                                               const int8_t* __restrict__ l,
                                                               const uint8_t* __restrict__ skey, uint8_t* slot,
                                                               uint32_t d, FetchScratch hv, FetchEmit em) {
  __shared__ uint32_t rec[kFpTileNodes * kShamapRecordWords];
  __shared__ uint32_t node_pos[kFpTileNodes];
  __shared__ uint32_t node_leaf[kFpTileNodes];
  __shared__ uint32_t node_row[kFpTileNodes];
  __shared__ uint32_t wave_nodes[kFpBlock / 64];
  __shared__ uint32_t wave_keep[kFpBlock / 64];
  __shared__ uint32_t tile_base[1];
  const uint32_t nodes = hdr[d];
  if (nodes == 0) return;  // uniform: no node at this depth
  const uint32_t m = hdr[kShamapHdrDistinct];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t chunks = (m + kFpBlock - 1) / kFpBlock;
  uint32_t want = (nodes + kFpSpansWanted - 1) / kFpSpansWanted;
  if (want > kFpTileNodes) want = kFpTileNodes;
  uint32_t per = (uint32_t)(((uint64_t)chunks * want) / nodes);
  if (per == 0) per = 1;
  if (per > kFpSpanChunksMax) per = kFpSpanChunksMax;
  const uint32_t spans = (chunks + per - 1) / per;
  for (uint32_t span = blockIdx.x; span < spans; span += gridDim.x) {
    const uint32_t first = span * per, past = first + per < chunks ? first + per : chunks;
    uint32_t count = 0;  // uniform: nodes listed and not yet hashed
    for (uint32_t ch = first; ch < past; ++ch) {
      const uint32_t i = ch * kFpBlock + tid;
      bool starts = false;
      if (i < m) starts = shamap_starts_node(i ? (int32_t)l[i - 1] : -1, (int32_t)l[i], (int32_t)d);
      const uint64_t sw = __ballot(starts);
      if (lane == 0) wave_nodes[wave] = (uint32_t)__popcll(sw);
      __syncthreads();
      uint32_t base = 0, here = 0;  // here <= 128: two starts are never adjacent
#pragma unroll
      for (uint32_t v = 0; v < kFpBlock / 64; ++v) {
        if (v < wave) base += wave_nodes[v];
        here += wave_nodes[v];
      }
      if (count + here > kFpTileNodes) {  // uniform
        fetch_flush(rec, node_pos, count, m, skey, slot, d, l, hv, em, node_leaf, node_row, wave_keep, tile_base);
        count = 0;
      }
      if (starts) {
        const uint32_t k = count + base + (uint32_t)__popcll(sw & ((1ull << lane) - 1ull));
        if (k < kFpTileNodes) node_pos[k] = i;  // always
      }
      count += here;
      if (count > kFpTileNodes) count = kFpTileNodes;  // never
      __syncthreads();  // wave_nodes is reused by the next chunk
    }
    if (count)
      fetch_flush(rec, node_pos, count, m, skey, slot, d, l, hv, em, node_leaf, node_row, wave_keep, tile_base);
  }
}

// 4. one depth of the top, both trees side by side: `nodes` prefixes of length
// `depth` from 16 children each, 64 prefixes to a workgroup of two waves.
// have_cnt null: no tree.  Want's prefix that is an inner node is a candidate,
// and is stored unless have holds the same.
__global__ __launch_bounds__(128) void fetch_top_kernel(const uint32_t* __restrict__ want_cnt,
                                                        const uint32_t* __restrict__ want_h,
                                                        const uint32_t* __restrict__ have_cnt,
                                                        const uint32_t* __restrict__ have_h, uint32_t nodes,
                                                        uint32_t depth, uint32_t* __restrict__ out_want_cnt,
                                                        uint32_t* __restrict__ out_want_h,
                                                        uint32_t* __restrict__ out_have_cnt,
                                                        uint32_t* __restrict__ out_have_h, FetchEmit em) {
  // Two waves: wave 0 folds want's 64 prefixes, wave 1 have's, side by side.  A
  // lane's record is 129 dwords from the next, so a wave hashes out of 64
  // different banks; have's values cross to wave 0 through have_val.
  __shared__ uint32_t recs[128 * kShamapRecordWords];
  __shared__ uint32_t have_val[64 * 9];
  const uint32_t lane = threadIdx.x & 63u;
  const bool have_side = threadIdx.x >= 64u;  // uniform per wave
  uint32_t* const rec = recs + threadIdx.x * kShamapRecordWords;
  const uint32_t t = blockIdx.x * 64 + lane;
  const bool root = depth == 0;
  uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, c = 0;
  if (t < nodes) {
    if (!have_side) {
      c = shamap_fetch_top_value(want_cnt + 16 * t, want_h + 128 * (size_t)t, root, rec, h);
    } else if (have_cnt) {
      c = shamap_fetch_top_value(have_cnt + 16 * t, have_h + 128 * (size_t)t, root, rec, h);
    }
    uint32_t* const oc = have_side ? out_have_cnt : out_want_cnt;
    uint32_t* const oh = have_side ? out_have_h : out_want_h;
    oc[t] = c;
    for (uint32_t i = 0; i < 8; ++i) oh[8 * t + i] = h[i];
  }
  if (have_side) {
    have_val[9 * lane] = c;
    for (uint32_t i = 0; i < 8; ++i) have_val[9 * lane + 1 + i] = h[i];
  }
  __syncthreads();
  if (have_side) return;
  bool candidate = false, keep = false;
  if (t < nodes) {
    uint32_t hh[8];
    for (uint32_t i = 0; i < 8; ++i) hh[i] = have_val[9 * lane + 1 + i];
    candidate = shamap_fetch_top_inner(c, root);
    keep = candidate && shamap_fetch_top_keeps(h, have_val[9 * lane], hh, root);
  }
  fp_count(candidate, &em.fh[kFhCandidates]);
  fp_count(candidate && !keep, &em.fh[kFhSuppressed]);
  if (!keep) return;
  const uint32_t row = atomicAdd(&em.fh[kFhEmitted], 1u);
  if (row >= em.max_nodes) return;
  // the body is the record want's value was hashed from; the rule writes it there again
  uint32_t* const body = rec + 1;
  uint32_t id[8];
  const uint32_t leaf = shamap_tree_top_node(want_cnt + 16 * t, want_h + 128 * (size_t)t, depth, t, body, id);
  fp_st8(em.hash, row, h);
  uint4* q = reinterpret_cast<uint4*>(em.body + 512 * (size_t)row);
  for (uint32_t i = 0; i < 32; ++i) q[i] = make_uint4(body[4 * i], body[4 * i + 1], body[4 * i + 2], body[4 * i + 3]);
  if (em.id) fp_st8(em.id, row, id);
  if (em.meta) em.meta[row] = shamap_node_meta(depth, leaf);
}

// 5. the count and the eight counts.  have_meta null: no tree.
__global__ __launch_bounds__(64) void fetch_finish_kernel(const uint32_t* __restrict__ fh,
                                                          const uint32_t* __restrict__ want_hdr,
                                                          const uint32_t* __restrict__ have_hdr,
                                                          const uint32_t* __restrict__ want_meta, uint32_t cap_want,
                                                          const uint32_t* __restrict__ have_meta, uint32_t cap_have,
                                                          uint32_t* __restrict__ count,
                                                          uint32_t* __restrict__ counts) {
  if (threadIdx.x != 0) return;
  *count = fh[kFhEmitted];
  if (!counts) return;
  counts[0] = fh[kFhEmitted];
  counts[1] = fh[kFhBuckets];
  counts[2] = want_hdr[kShamapHdrDistinct];
  counts[3] = have_hdr[kShamapHdrDistinct];
  counts[4] = fh[kFhCandidates];
  counts[5] = fh[kFhSuppressed];
  counts[6] = shamap_tree_readable(want_meta[0], cap_want);
  counts[7] = have_meta ? shamap_tree_readable(have_meta[0], cap_have) : 0u;
}

}  // namespace

size_t shamap_fetch_workspace_bytes(size_t want_bound, size_t have_bound, size_t temp_bytes) {
  return FetchWs(nullptr, want_bound, have_bound, temp_bytes).bytes;
}

#define FP_TRY(expr)                              \
  do {                                            \
    if (fault && fault()) return hipErrorUnknown; \
    const hipError_t e_ = (expr);                 \
    if (e_ != hipSuccess) return e_;              \
  } while (0)

#define FP_LAUNCH(kernel, grid, block, ...)                                      \
  do {                                                                           \
    if (fault && fault()) return hipErrorUnknown;                                \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
    const hipError_t e_ = hipGetLastError();                                     \
    if (e_ != hipSuccess) return e_;                                             \
  } while (0)

#define FP_RC(expr)                  \
  do {                               \
    const hipError_t e_ = (expr);    \
    if (e_ != hipSuccess) return e_; \
  } while (0)

hipError_t launch_shamap_tree_fetch_pack(const TreeGen& want, uint32_t cap_want, uint32_t want_bound,
                                         const TreeGen* have, uint32_t cap_have, uint32_t have_bound,
                                         const ShamapEmit& emit, uint32_t* counts, void* ws, size_t temp_bytes,
                                         bool (*fault)(), const PhaseClock* clock, hipStream_t stream) {
  if (!ws || ((uintptr_t)ws & 255u) || cap_want == 0 || want_bound > cap_want) return hipErrorInvalidValue;
  if (have && (cap_have == 0 || have_bound > cap_have)) return hipErrorInvalidValue;
  if (!emit.hash || !emit.body || !emit.count) return hipErrorInvalidValue;
  if ((((uintptr_t)emit.hash | (uintptr_t)emit.body | (uintptr_t)emit.id) & 15u) ||
      (((uintptr_t)emit.meta | (uintptr_t)emit.count | (uintptr_t)counts) & 3u))
    return hipErrorInvalidValue;
  if (!have) have_bound = 0;
  // have's keys are only ever asked by want's nodes
  const bool want_rows = want_bound != 0, have_rows = want_rows && have_bound != 0;
  const FetchWs w(ws, want_bound, have_bound, temp_bytes);
  const FetchEmit em{emit.hash, emit.body, emit.id, emit.meta, emit.max_nodes, w.fh};
  const uint32_t gb = kTreeBuckets / kFpBlock;
  const uint32_t* const no_words = nullptr;
  if (clock) clock->mark(clock->ctx, stream, 0);
  FP_TRY(hipMemsetAsync(w.fh, 0, w.cleared(), stream));
  // 1. buckets
  FP_LAUNCH(fetch_buckets_kernel, gb, kFpBlock, want.bcnt, want.bh, have ? have->bcnt : no_words,
            have ? have->bh : no_words, w.sz_w, w.sz_h, w.fh);
  if (want_rows) {
    // 2. gather
    FP_RC(shamap_exclusive_scan(w.temp, temp_bytes, want.bcnt, w.begin_w, kTreeBuckets, fault, stream));
    FP_RC(shamap_exclusive_scan(w.temp, temp_bytes, w.sz_w, w.off_w, kTreeBuckets, fault, stream));
    FP_LAUNCH(fetch_gather_kernel, grid_of(want_bound), kFpBlock, want.key, want.leaf, want.bcnt, want.meta, cap_want,
              w.begin_w, w.sz_w, w.off_w, want_bound, w.w.hdr, w.w.skey, w.w.slot);
    FP_RC(launch_shamap_neighbours(w.w.hdr, w.w.l, w.w.skey, want_bound, fault, stream));
    if (have_rows) {
      FP_RC(shamap_exclusive_scan(w.temp, temp_bytes, have->bcnt, w.begin_h, kTreeBuckets, fault, stream));
      FP_RC(shamap_exclusive_scan(w.temp, temp_bytes, w.sz_h, w.off_h, kTreeBuckets, fault, stream));
      FP_LAUNCH(fetch_gather_kernel, grid_of(have_bound), kFpBlock, have->key, have->leaf, have->bcnt, have->meta,
                cap_have, w.begin_h, w.sz_h, w.off_h, have_bound, w.h.hdr, w.h.skey, w.h.slot);
      FP_RC(launch_shamap_neighbours(w.h.hdr, w.h.l, w.h.skey, have_bound, fault, stream));
    }
  }
  if (clock) clock->mark(clock->ctx, stream, 1);
  if (want_rows) {
    // 3. levels: have's depth d is hashed just before want's asks for it
    FetchScratch hv = w.h;
    if (!have_rows) hv.hdr = nullptr;
    const uint32_t g = grid_of(want_bound), lg = g < kFpLevelGrid ? g : kFpLevelGrid;
    for (int d = (int)kShamapDepths - 1; d >= (int)kTreeBucketDepth; --d) {
      if (have_rows)
        FP_RC(launch_shamap_level(w.h.hdr, w.h.l, w.h.skey, w.h.slot, have_bound, (uint32_t)d, fault, stream));
      FP_LAUNCH(fetch_level_kernel, lg, kFpBlock, w.w.hdr, w.w.l, w.w.skey, w.w.slot, (uint32_t)d, hv, em);
    }
  }
  if (clock) clock->mark(clock->ctx, stream, 2);
  // 4. top: the prefixes of length 3, 2, 1 and the root
  {
    const uint32_t *wc = want.bcnt, *wh = want.bh, *hc = have ? have->bcnt : no_words, *hh = have ? have->bh : no_words;
    uint32_t o = 0;
    for (uint32_t depth = kTreeBucketDepth; depth-- > 0;) {
      const uint32_t nodes = 1u << (4 * depth);
      FP_LAUNCH(fetch_top_kernel, (nodes + 63) / 64, 128, wc, wh, hc, hh, nodes, depth, w.topcnt_w + o,
                w.toph_w + 8 * o, w.topcnt_h + o, w.toph_h + 8 * o, em);
      wc = w.topcnt_w + o, wh = w.toph_w + 8 * o;
      if (have) hc = w.topcnt_h + o, hh = w.toph_h + 8 * o;
      o += nodes;
    }
  }
  // 5. finish
  FP_LAUNCH(fetch_finish_kernel, 1, 64, w.fh, w.w.hdr, w.h.hdr, want.meta, cap_want, have ? have->meta : no_words,
            cap_have, emit.count, counts);
  if (clock) {
    clock->mark(clock->ctx, stream, 3);
    clock->mark(clock->ctx, stream, 4);
  }
  return hipSuccess;
}

}  // namespace stl
