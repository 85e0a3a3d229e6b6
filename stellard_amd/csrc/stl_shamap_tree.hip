// stl_shamap_tree.hip -- gfx950 kernels of the resident SHAMap
// (stl_shamap_tree_*): a tree's sorted keys and leaf hashes stay in HBM, a
// batch of changes (set or delete per row) is merged in, and only the buckets
// the batch touches are rehashed (stl_shamap_tree_core.h has the rules).
//
// One apply, all on the caller's stream, one generation read and another written:
//   1. changes   the batch's keys through the sort passes of stl_shamap.hip;
//                the last of equal keys is a change (head rule, scan, compact)
//   2. locate    one lane per change bisects the resident keys: position, found,
//                delta; the deltas are scanned; the change's bucket is marked dirty
//   3. merge     one lane per resident item finds the changes before it from their
//                positions and copies itself to i + scan (unless deleted; with the
//                change's leaf hash when replaced); one lane per inserted change
//                writes it to pos + scan.  O(items) bytes move per apply.
//   4. bounds    65,537 lanes bisect the new keys on their 16-bit prefix
//   5. subtrees  the dirty buckets' sizes are scanned and their rows gathered, in
//                order, into the scratch; the neighbour and level kernels of
//                stl_shamap.hip run depths 63 down to 4 over it
//   6. top       a dirty bucket's value is (size, scratch slot of its first key),
//                a clean one's is copied; four launches fold the 65,536 values
//                into the root
//   7. finish    root and counts -- the only launch that writes the caller's outputs
//
// Every count is read on the device; the grids come from host-known bounds
// (rows of the batch, a bound of the item count).  Every store into a
// generation or the scratch is guarded by the capacity.
//
// A fork (stl_shamap_tree_fork*) is the same sequence with the generation read
// belonging to another tree than the one written: every read of `from` is
// clamped by that tree's capacity (shamap_tree_readable), every store guarded by
// the written tree's, and the work areas are the written tree's.  A fork of no
// rows is tree_snapshot_kernel: a copy by the count, nothing sorted or hashed.
#include "stl_shamap_tree.h"

#include "stl_shamap.h"
#include "stl_shamap_tree_core.h"

namespace stl {

namespace {

constexpr uint32_t kTrBlock = 256;
// header words of the fixed work area
constexpr uint32_t kWhChanges = 0, kWhInserted = 1, kWhReplaced = 2, kWhDeleted = 3, kWhAbsent = 4, kWhDirty = 6,
                   kWhGathered = 7, kWhWords = 64;

__device__ __forceinline__ void tr_st8(uint8_t* p, size_t row, const uint32_t k[8]) {
  uint4* q = reinterpret_cast<uint4*>(p + 32 * row);
  q[0] = make_uint4(k[0], k[1], k[2], k[3]);
  q[1] = make_uint4(k[4], k[5], k[6], k[7]);
}

__device__ __forceinline__ void tr_count(bool v, uint32_t* word) {
  const uint64_t b = __ballot(v);
  if ((threadIdx.x & 63u) == 0 && b != 0) atomicAdd(word, (uint32_t)__popcll(b));
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
uint32_t grid_of(uint32_t n) { return (n + kTrBlock - 1) / kTrBlock; }

// The work areas' parts, in order.
struct TreeFixed {
  uint32_t *wh, *dirty, *lb, *sz, *off, *topcnt, *toph, *topdirty;
  size_t bytes;
  explicit TreeFixed(void* base) {
    uint8_t* p = static_cast<uint8_t*>(base);
    size_t o = 0;
    auto take = [&](size_t b) {
      uint32_t* q = reinterpret_cast<uint32_t*>(p + o);
      o += up256(b);
      return q;
    };
    wh = take(4 * kWhWords);  // the header and the dirty flags are cleared by one memset
    dirty = take(4 * kTreeBuckets);
    lb = take(4 * (kTreeBuckets + 1));
    sz = take(4 * kTreeBuckets);
    off = take(4 * kTreeBuckets);
    topcnt = take(4 * kTreeTopValues);
    toph = take(32 * kTreeTopValues);
    topdirty = take(4 * kTreeTopValues);  // a dirty bucket lies below the prefix (the storing apply alone)
    bytes = o;
  }
};

struct TreeBatch {
  uint8_t *ckey, *cleaf, *code;
  uint32_t *pos, *delta, *scan;
  size_t bytes;
  TreeBatch(void* base, size_t n) {
    uint8_t* p = static_cast<uint8_t*>(base);
    size_t o = 0;
    auto take = [&](size_t b) {
      uint8_t* q = p + o;
      o += up256(b);
      return q;
    };
    ckey = take(32 * n);
    cleaf = take(32 * n);
    code = take(4 * n);
    pos = reinterpret_cast<uint32_t*>(take(4 * n));
    delta = reinterpret_cast<uint32_t*>(take(4 * n));
    scan = reinterpret_cast<uint32_t*>(take(4 * n));
    bytes = o;
  }
};

struct TreeScratch {
  uint32_t* hdr;
  int8_t* l;
  uint8_t *skey, *slot;
  size_t bytes;
  TreeScratch(void* base, size_t cap) {
    uint8_t* p = static_cast<uint8_t*>(base);
    size_t o = 0;
    auto take = [&](size_t b) {
      uint8_t* q = p + o;
      o += up256(b);
      return q;
    };
    hdr = reinterpret_cast<uint32_t*>(take(kShamapHeaderBytes));
    l = reinterpret_cast<int8_t*>(take(cap));
    skey = take(32 * cap);
    slot = take(32 * cap);
    bytes = o;
  }
};

// 1. flags[i] = sorted position i holds a change: the last of its key.
__global__ __launch_bounds__(kTrBlock) void tree_head_kernel(const uint8_t* __restrict__ key,
                                                             const uint32_t* __restrict__ perm, uint32_t n,
                                                             uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * kTrBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t cp = 0;
  if (i + 1 < n) {
    uint32_t a[8], b[8];
    shamap_load_key(a, key, perm[i]);
    shamap_load_key(b, key, perm[i + 1]);
    cp = shamap_common_prefix(a, b);
  }
  flags[i] = shamap_tree_head(i + 1 == n, cp) ? 1u : 0u;
}

// Change j (flags, idx: its number) -> ckey[j], cleaf[j], code[j]; the last
// position writes the number of changes.
__global__ __launch_bounds__(kTrBlock) void tree_compact_kernel(
    const uint8_t* __restrict__ key, const uint8_t* __restrict__ leaf, const uint8_t* __restrict__ op,
    const uint32_t* __restrict__ perm, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ idx, uint32_t n,
    uint8_t* __restrict__ ckey, uint8_t* __restrict__ cleaf, uint8_t* __restrict__ code, uint32_t* __restrict__ wh) {
  const uint32_t i = blockIdx.x * kTrBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t f = flags[i], j = idx[i];
  if (i == n - 1) wh[kWhChanges] = j + f;
  if (!f || j >= n) return;
  const uint32_t row = perm[i];
  const bool del = op && op[row] != 0;
  uint32_t k[8];
  shamap_load_key(k, key, row);
  tr_st8(ckey, j, k);
  if (leaf && !del) shamap_load_key(k, leaf, row);  // a delete's leaf hash is never read
  tr_st8(cleaf, j, k);
  code[j] = del ? (uint8_t)kTreeOpDelete : (uint8_t)0;
}

// 2. position, found and delta of every change; its bucket becomes dirty.
__global__ __launch_bounds__(kTrBlock) void tree_locate_kernel(const uint8_t* __restrict__ rkey,
                                                               const uint32_t* __restrict__ meta, uint32_t from_cap,
                                                               const uint8_t* __restrict__ ckey,
                                                               uint8_t* __restrict__ code, uint32_t n,
                                                               uint32_t* __restrict__ pos, uint32_t* __restrict__ delta,
                                                               uint32_t* __restrict__ dirty, uint32_t* wh) {
  const uint32_t j = blockIdx.x * kTrBlock + threadIdx.x;
  const uint32_t k = wh[kWhChanges] < n ? wh[kWhChanges] : n;
  const uint32_t m = shamap_tree_readable(meta[0], from_cap);
  bool ins = false, rep = false, del = false, absent = false;
  if (j < k) {
    uint32_t key[8];
    shamap_load_key(key, ckey, j);
    bool found = false;
    const uint32_t p = shamap_tree_lower_bound(rkey, m, key, &found);
    const bool is_del = (code[j] & kTreeOpDelete) != 0;
    pos[j] = p;
    delta[j] = (uint32_t)shamap_tree_delta(is_del, found);
    code[j] = (uint8_t)((is_del ? kTreeOpDelete : 0u) | (found ? kTreeFound : 0u));
    dirty[shamap_tree_bucket(key)] = 1u;
    ins = !is_del && !found;
    rep = !is_del && found;
    del = is_del && found;
    absent = is_del && !found;
  } else if (j < n) {
    delta[j] = 0u;  // the scan runs over all n words
  }
  tr_count(ins, &wh[kWhInserted]);
  tr_count(rep, &wh[kWhReplaced]);
  tr_count(del, &wh[kWhDeleted]);
  tr_count(absent, &wh[kWhAbsent]);
}

// 3a. resident item i -> its place in the other generation.
__global__ __launch_bounds__(kTrBlock) void tree_merge_items_kernel(
    const uint8_t* __restrict__ rkey, const uint8_t* __restrict__ rleaf, const uint32_t* __restrict__ meta,
    uint32_t from_cap, uint32_t cap, const uint32_t* __restrict__ pos, const uint8_t* __restrict__ code,
    const uint32_t* __restrict__ scan, const uint8_t* __restrict__ cleaf, const uint32_t* __restrict__ wh, uint32_t n,
    uint8_t* __restrict__ nkey, uint8_t* __restrict__ nleaf) {
  const uint32_t i = blockIdx.x * kTrBlock + threadIdx.x;
  const uint32_t m = shamap_tree_readable(meta[0], from_cap);
  if (i >= m) return;
  const uint32_t k = wh[kWhChanges] < n ? wh[kWhChanges] : n;
  bool hit = false;
  const uint32_t r = shamap_tree_changes_before(pos, code, k, i, &hit);
  if (hit && (code[r] & kTreeOpDelete)) return;
  const uint32_t before = r < k ? scan[r] : wh[kWhInserted] - wh[kWhDeleted];
  const uint32_t dst = shamap_tree_item_dest(i, before);
  if (dst >= cap) return;  // never: the host admits a batch only when bound + n <= the written tree's capacity
  uint32_t v[8];
  shamap_load_key(v, rkey, i);
  tr_st8(nkey, dst, v);
  if (hit) shamap_load_key(v, cleaf, r); else shamap_load_key(v, rleaf, i);
  tr_st8(nleaf, dst, v);
}

// 3b. inserted change j -> its place.
__global__ __launch_bounds__(kTrBlock) void tree_merge_changes_kernel(
    const uint8_t* __restrict__ ckey, const uint8_t* __restrict__ cleaf, const uint8_t* __restrict__ code,
    const uint32_t* __restrict__ pos, const uint32_t* __restrict__ scan, const uint32_t* __restrict__ wh, uint32_t n,
    uint32_t cap, uint8_t* __restrict__ nkey, uint8_t* __restrict__ nleaf) {
  const uint32_t j = blockIdx.x * kTrBlock + threadIdx.x;
  const uint32_t k = wh[kWhChanges] < n ? wh[kWhChanges] : n;
  if (j >= k || (code[j] & (kTreeOpDelete | kTreeFound))) return;
  const uint32_t dst = shamap_tree_insert_dest(pos[j], scan[j]);
  if (dst >= cap) return;  // never
  uint32_t v[8];
  shamap_load_key(v, ckey, j);
  tr_st8(nkey, dst, v);
  shamap_load_key(v, cleaf, j);
  tr_st8(nleaf, dst, v);
}

// 4. the new count, and where every bucket begins in the new keys.
__global__ __launch_bounds__(kTrBlock) void tree_bounds_kernel(const uint8_t* __restrict__ nkey,
                                                               const uint32_t* __restrict__ meta_from,
                                                               uint32_t* __restrict__ meta_to,
                                                               const uint32_t* __restrict__ wh, uint32_t from_cap,
                                                               uint32_t cap, uint32_t* __restrict__ lb) {
  const uint32_t b = blockIdx.x * kTrBlock + threadIdx.x;
  if (b > kTreeBuckets) return;
  uint32_t m = shamap_tree_readable(meta_from[0], from_cap) + wh[kWhInserted] - wh[kWhDeleted];
  if (m > cap) m = cap;  // never
  lb[b] = shamap_tree_bucket_begin(nkey, m, b);
  if (b == 0) meta_to[0] = m;
}

// 5a. the dirty buckets' sizes.
__global__ __launch_bounds__(kTrBlock) void tree_sizes_kernel(const uint32_t* __restrict__ dirty,
                                                              const uint32_t* __restrict__ lb,
                                                              uint32_t* __restrict__ sz, uint32_t* wh) {
  const uint32_t b = blockIdx.x * kTrBlock + threadIdx.x;  // the grid is kTreeBuckets lanes exactly
  const bool d = dirty[b] != 0;
  sz[b] = d ? lb[b + 1] - lb[b] : 0u;
  tr_count(d, &wh[kWhDirty]);
}

// 5b. scratch position p <- the row of its dirty bucket.
__global__ __launch_bounds__(kTrBlock) void tree_gather_kernel(const uint8_t* __restrict__ nkey,
                                                               const uint8_t* __restrict__ nleaf,
                                                               const uint32_t* __restrict__ lb,
                                                               const uint32_t* __restrict__ sz,
                                                               const uint32_t* __restrict__ off, uint32_t cap,
                                                               uint32_t* __restrict__ hdr, uint8_t* __restrict__ skey,
                                                               uint8_t* __restrict__ slot, uint32_t* __restrict__ wh) {
  const uint32_t p = blockIdx.x * kTrBlock + threadIdx.x;
  uint32_t total = off[kTreeBuckets - 1] + sz[kTreeBuckets - 1];
  if (total > cap) total = cap;  // never
  if (p == 0) {
    hdr[kShamapHdrDistinct] = total;
    wh[kWhGathered] = total;
  }
  if (p >= total) return;
  uint32_t lo = 0, hi = kTreeBuckets;  // the first bucket whose offset is past p
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= p) lo = mid + 1; else hi = mid;
  }
  const uint32_t b = lo - 1;  // off[0] = 0 <= p, and the last bucket at an offset is the one with rows
  const uint32_t src = lb[b] + (p - off[b]);
  if (src >= cap) return;  // never
  uint32_t v[8];
  shamap_load_key(v, nkey, src);
  tr_st8(skey, p, v);
  shamap_load_key(v, nleaf, src);
  tr_st8(slot, p, v);
}

// 6a. the bucket values of the new generation.
__global__ __launch_bounds__(kTrBlock) void tree_bucket_kernel(const uint32_t* __restrict__ dirty,
                                                               const uint32_t* __restrict__ sz,
                                                               const uint32_t* __restrict__ off,
                                                               const uint8_t* __restrict__ slot, uint32_t cap,
                                                               uint32_t from_cap,
                                                               const uint32_t* __restrict__ from_cnt,
                                                               const uint32_t* __restrict__ from_h,
                                                               uint32_t* __restrict__ to_cnt,
                                                               uint32_t* __restrict__ to_h) {
  const uint32_t b = blockIdx.x * kTrBlock + threadIdx.x;  // kTreeBuckets lanes exactly
  uint32_t c, h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (dirty[b]) {
    c = sz[b];
    if (c && off[b] < cap) shamap_load_key(h, slot, off[b]);
  } else {
    c = shamap_tree_readable(from_cnt[b], from_cap);  // a clean bucket holds what it held
    shamap_load_key(h, reinterpret_cast<const uint8_t*>(from_h), b);
  }
  to_cnt[b] = c;
  tr_st8(reinterpret_cast<uint8_t*>(to_h), b, h);
}

// What the storing top kernel is given besides the values: the children's
// "a dirty bucket lies below" words and where its own go (null at the root),
// the prefixes' length, ShamapEmit's arrays and the word the rows are numbered from.
struct TopEmit {
  const uint32_t* child_dirty;
  uint32_t* out_dirty;
  uint32_t depth;
  uint8_t* hash;
  uint8_t* body;
  uint8_t* id;
  uint32_t* meta;
  uint32_t max_nodes;
  uint32_t* counter;
};

// 6b. one depth of the top: `nodes` values from 16 children each.  kEmit: a
// prefix that is an inner node above a dirty bucket is also stored, one row
// number per node from the counter the level kernel has used; every store is
// guarded by the row number being below max_nodes.
template <bool kEmit>
__global__ __launch_bounds__(64) void tree_top_kernel(const uint32_t* __restrict__ child_cnt,
                                                      const uint32_t* __restrict__ child_h, uint32_t nodes, bool root,
                                                      uint32_t* __restrict__ out_cnt, uint32_t* __restrict__ out_h,
                                                      TopEmit em) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= nodes) return;
  uint32_t h[8];
  const uint32_t c = shamap_tree_top_value(child_cnt + 16 * t, child_h + 128 * (size_t)t, root, h);
  if (out_cnt) out_cnt[t] = c;
  for (uint32_t i = 0; i < 8; ++i) out_h[8 * t + i] = h[i];
  if constexpr (kEmit) {
    uint32_t below = 0;
    for (uint32_t k = 0; k < kShamapBranches; ++k) below |= em.child_dirty[16 * t + k];
    if (em.out_dirty) em.out_dirty[t] = below ? 1u : 0u;
    if (!shamap_tree_top_emits(c, root, below != 0)) return;
    const uint32_t row = atomicAdd(em.counter, 1u);
    if (row >= em.max_nodes) return;
    uint32_t body[16 * kShamapKeyWords], id[8];
    const uint32_t leaf = shamap_tree_top_node(child_cnt + 16 * t, child_h + 128 * (size_t)t, em.depth, t, body, id);
    tr_st8(em.hash, row, h);
    uint4* q = reinterpret_cast<uint4*>(em.body + 512 * (size_t)row);
    for (uint32_t i = 0; i < 32; ++i) q[i] = make_uint4(body[4 * i], body[4 * i + 1], body[4 * i + 2], body[4 * i + 3]);
    if (em.id) tr_st8(em.id, row, id);
    if (em.meta) em.meta[row] = shamap_node_meta(em.depth, leaf);
  }
}

// 7. root and counts; the number of stored nodes (emitted: its counter, or null
// for none) -> node_count (or null).
__global__ __launch_bounds__(64) void tree_finish_kernel(const uint32_t* __restrict__ meta,
                                                         const uint32_t* __restrict__ wh, uint32_t n,
                                                         uint32_t* __restrict__ root, uint32_t* __restrict__ counts,
                                                         const uint32_t* __restrict__ emitted,
                                                         uint32_t* __restrict__ node_count) {
  const uint32_t t = threadIdx.x;
  if (t == 0 && node_count) *node_count = emitted ? *emitted : 0u;
  if (t < 8) root[t] = meta[kTreeMetaRoot + t];
  if (t == 0 && counts) {
    counts[0] = meta[0];
    counts[1] = wh ? wh[kWhInserted] : 0u;
    counts[2] = wh ? wh[kWhReplaced] : 0u;
    counts[3] = wh ? wh[kWhDeleted] : 0u;
    counts[4] = wh ? wh[kWhAbsent] : 0u;
    counts[5] = wh ? n - wh[kWhChanges] : 0u;
    counts[6] = wh ? wh[kWhDirty] : 0u;
    counts[7] = wh ? wh[kWhGathered] : 0u;
  }
}

__global__ __launch_bounds__(kTrBlock) void tree_export_kernel(const uint8_t* __restrict__ rkey,
                                                               const uint8_t* __restrict__ rleaf,
                                                               const uint32_t* __restrict__ meta, uint32_t rows,
                                                               uint8_t* __restrict__ key, uint8_t* __restrict__ leaf,
                                                               uint32_t* __restrict__ items) {
  const uint32_t i = blockIdx.x * kTrBlock + threadIdx.x;
  const uint32_t m = meta[0];
  if (i == 0 && items) *items = m;
  if (i >= m || i >= rows) return;
  uint32_t v[8];
  if (key) {
    shamap_load_key(v, rkey, i);
    tr_st8(key, i, v);
  }
  if (leaf) {
    shamap_load_key(v, rleaf, i);
    tr_st8(leaf, i, v);
  }
}

// The snapshot (a fork of no rows): one generation copied into another tree's,
// in 16-byte units, lane t the t-th unit of each array -- a wave's load or store
// is 1 KiB in a row.  The keys and the leaf hashes follow the count read here
// (two units per row), under the source's clamp and the destination's guard;
// the bucket values are 16,384 + 131,072 units, the meta words four, and word 0
// of those is the count that was copied.
constexpr uint32_t kSnapFixedUnits = 2 * kTreeBuckets;
__global__ __launch_bounds__(kTrBlock) void tree_snapshot_kernel(TreeGen from, uint32_t from_cap, TreeGen to,
                                                                 uint32_t cap) {
  const uint32_t t = blockIdx.x * kTrBlock + threadIdx.x;
  const uint32_t m = shamap_tree_snapshot_rows(from.meta[0], from_cap, cap);
  if (t < 2 * m) {
    const uint4 k = reinterpret_cast<const uint4*>(from.key)[t];
    const uint4 l = reinterpret_cast<const uint4*>(from.leaf)[t];
    reinterpret_cast<uint4*>(to.key)[t] = k;
    reinterpret_cast<uint4*>(to.leaf)[t] = l;
  }
  if (t < kSnapFixedUnits) reinterpret_cast<uint4*>(to.bh)[t] = reinterpret_cast<const uint4*>(from.bh)[t];
  if (t < kTreeBuckets / 4) reinterpret_cast<uint4*>(to.bcnt)[t] = reinterpret_cast<const uint4*>(from.bcnt)[t];
  if (t < kTreeMetaWords / 4) {
    uint4 w = reinterpret_cast<const uint4*>(from.meta)[t];
    if (t == 0) w.x = m;
    reinterpret_cast<uint4*>(to.meta)[t] = w;
  }
}

}  // namespace

size_t shamap_tree_gen_fixed_bytes() { return up256(4 * kTreeBuckets) + up256(32 * kTreeBuckets) + up256(4 * kTreeMetaWords); }
size_t shamap_tree_fixed_bytes() { return TreeFixed(nullptr).bytes; }
size_t shamap_tree_batch_bytes(size_t n) { return TreeBatch(nullptr, n).bytes; }
size_t shamap_tree_scratch_bytes(size_t capacity) { return TreeScratch(nullptr, capacity).bytes; }

#define TR_TRY(expr)                              \
  do {                                            \
    if (fault && fault()) return hipErrorUnknown; \
    const hipError_t e_ = (expr);                 \
    if (e_ != hipSuccess) return e_;              \
  } while (0)

#define TR_LAUNCH(kernel, grid, block, ...)                                      \
  do {                                                                           \
    if (fault && fault()) return hipErrorUnknown;                                \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
    const hipError_t e_ = hipGetLastError();                                     \
    if (e_ != hipSuccess) return e_;                                             \
  } while (0)

#define TR_RC(expr)                  \
  do {                               \
    const hipError_t e_ = (expr);    \
    if (e_ != hipSuccess) return e_; \
  } while (0)

hipError_t launch_shamap_tree_locate(const TreeApply& a, const uint8_t* key, const uint8_t* leaf, const uint8_t* op,
                                     uint32_t n, bool (*fault)(), const PhaseClock* clock, hipStream_t stream) {
  if (n == 0 || !key || !a.fixed || !a.batch || !a.scratch || !a.sort_ws) return hipErrorInvalidValue;
  if (((uintptr_t)key & 15u) || ((uintptr_t)leaf & 15u)) return hipErrorInvalidValue;
  if (a.capacity == 0 || a.from_capacity == 0 || a.items_bound > a.from_capacity || n > a.capacity)
    return hipErrorInvalidValue;
  const TreeFixed f(a.fixed);
  const TreeBatch b(a.batch, n);
  const uint32_t gn = grid_of(n);
  if (clock) clock->mark(clock->ctx, stream, 0);
  TR_TRY(hipMemsetAsync(f.wh, 0, (size_t)(reinterpret_cast<uint8_t*>(f.dirty) - reinterpret_cast<uint8_t*>(f.wh)) +
                                     4 * kTreeBuckets, stream));
  // 1. changes
  ShamapSorted so{};
  TR_RC(launch_shamap_sort(key, n, a.sort_ws, a.temp_bytes, fault, stream, &so));
  TR_LAUNCH(tree_head_kernel, gn, kTrBlock, key, so.perm, n, so.flags);
  TR_RC(shamap_exclusive_scan(so.temp, a.temp_bytes, so.flags, so.idx, n, fault, stream));
  TR_LAUNCH(tree_compact_kernel, gn, kTrBlock, key, leaf, op, so.perm, so.flags, so.idx, n, b.ckey, b.cleaf, b.code,
            f.wh);
  // 2. locate
  TR_LAUNCH(tree_locate_kernel, gn, kTrBlock, a.from.key, a.from.meta, a.from_capacity, b.ckey, b.code, n, b.pos,
            b.delta, f.dirty, f.wh);
  TR_RC(shamap_exclusive_scan(so.temp, a.temp_bytes, b.delta, b.scan, n, fault, stream));
  if (clock) clock->mark(clock->ctx, stream, 1);
  return hipSuccess;
}

const uint32_t* shamap_tree_change_counts(void* fixed) { return TreeFixed(fixed).wh; }

hipError_t launch_shamap_tree_merge(const TreeApply& a, uint32_t n, uint8_t* root, uint32_t* counts, bool (*fault)(),
                                    const PhaseClock* clock, hipStream_t stream, const ShamapEmit* emit) {
  if (n == 0 || !root || !a.fixed || !a.batch || !a.scratch || !a.sort_ws) return hipErrorInvalidValue;
  if (((uintptr_t)root & 3u) || ((uintptr_t)counts & 3u)) return hipErrorInvalidValue;
  if (a.capacity == 0 || a.from_capacity == 0 || a.items_bound > a.from_capacity || a.after_bound > a.capacity ||
      a.after_bound == 0)
    return hipErrorInvalidValue;
  const TreeFixed f(a.fixed);
  const TreeBatch b(a.batch, n);
  const TreeScratch s(a.scratch, a.capacity);
  const uint32_t cap = a.capacity, from_cap = a.from_capacity, after = a.after_bound;
  const uint32_t gn = grid_of(n), gb = kTreeBuckets / kTrBlock;
  void* temp = shamap_workspace_temp(n, a.sort_ws, a.temp_bytes);
  // 3. merge
  if (a.items_bound)
    TR_LAUNCH(tree_merge_items_kernel, grid_of(a.items_bound), kTrBlock, a.from.key, a.from.leaf, a.from.meta,
              from_cap, cap, b.pos, b.code, b.scan, b.cleaf, f.wh, n, a.to.key, a.to.leaf);
  TR_LAUNCH(tree_merge_changes_kernel, gn, kTrBlock, b.ckey, b.cleaf, b.code, b.pos, b.scan, f.wh, n, cap, a.to.key,
            a.to.leaf);
  if (clock) clock->mark(clock->ctx, stream, 2);
  // 4. bounds
  TR_LAUNCH(tree_bounds_kernel, gb + 1, kTrBlock, a.to.key, a.from.meta, a.to.meta, f.wh, from_cap, cap, f.lb);
  // 5. subtrees
  TR_LAUNCH(tree_sizes_kernel, gb, kTrBlock, f.dirty, f.lb, f.sz, f.wh);
  TR_RC(shamap_exclusive_scan(temp, a.temp_bytes, f.sz, f.off, kTreeBuckets, fault, stream));
  TR_TRY(hipMemsetAsync(s.hdr, 0, kShamapHeaderBytes, stream));
  TR_LAUNCH(tree_gather_kernel, grid_of(after), kTrBlock, a.to.key, a.to.leaf, f.lb, f.sz, f.off, cap, s.hdr, s.skey,
            s.slot, f.wh);
  TR_RC(launch_shamap_levels(s.hdr, s.l, s.skey, s.slot, after, kShamapDepths - 1, kTreeBucketDepth, fault, stream,
                             emit));
  if (clock) clock->mark(clock->ctx, stream, 3);
  // 6. bucket values and top
  TR_LAUNCH(tree_bucket_kernel, gb, kTrBlock, f.dirty, f.sz, f.off, s.slot, cap, from_cap, a.from.bcnt, a.from.bh,
            a.to.bcnt, a.to.bh);
  uint32_t* const no_words = nullptr;
  if (emit) {
    // the same four launches, storing: the row numbers go on from where the scratch's level launches stopped
    TopEmit te{f.dirty, f.topdirty, 3u, emit->hash, emit->body, emit->id, emit->meta, emit->max_nodes,
               s.hdr + kShamapHdrEmitted};
    TR_LAUNCH(tree_top_kernel<true>, 4096 / 64, 64, a.to.bcnt, a.to.bh, 4096u, false, f.topcnt, f.toph, te);
    te.child_dirty = f.topdirty, te.out_dirty = f.topdirty + 4096, te.depth = 2u;
    TR_LAUNCH(tree_top_kernel<true>, 256 / 64, 64, f.topcnt, f.toph, 256u, false, f.topcnt + 4096, f.toph + 8 * 4096,
              te);
    te.child_dirty = f.topdirty + 4096, te.out_dirty = f.topdirty + 4096 + 256, te.depth = 1u;
    TR_LAUNCH(tree_top_kernel<true>, 1, 64, f.topcnt + 4096, f.toph + 8 * 4096, 16u, false, f.topcnt + 4096 + 256,
              f.toph + 8 * (4096 + 256), te);
    te.child_dirty = f.topdirty + 4096 + 256, te.out_dirty = nullptr, te.depth = 0u;
    TR_LAUNCH(tree_top_kernel<true>, 1, 64, f.topcnt + 4096 + 256, f.toph + 8 * (4096 + 256), 1u, true, no_words,
              a.to.meta + kTreeMetaRoot, te);
  } else {
    const TopEmit te{};
    TR_LAUNCH(tree_top_kernel<false>, 4096 / 64, 64, a.to.bcnt, a.to.bh, 4096u, false, f.topcnt, f.toph, te);
    TR_LAUNCH(tree_top_kernel<false>, 256 / 64, 64, f.topcnt, f.toph, 256u, false, f.topcnt + 4096, f.toph + 8 * 4096,
              te);
    TR_LAUNCH(tree_top_kernel<false>, 1, 64, f.topcnt + 4096, f.toph + 8 * 4096, 16u, false, f.topcnt + 4096 + 256,
              f.toph + 8 * (4096 + 256), te);
    TR_LAUNCH(tree_top_kernel<false>, 1, 64, f.topcnt + 4096 + 256, f.toph + 8 * (4096 + 256), 1u, true, no_words,
              a.to.meta + kTreeMetaRoot, te);
  }
  // 7. finish
  TR_LAUNCH(tree_finish_kernel, 1, 64, a.to.meta, f.wh, n, reinterpret_cast<uint32_t*>(root), counts,
            emit ? s.hdr + kShamapHdrEmitted : no_words, emit ? emit->count : no_words);
  if (clock) clock->mark(clock->ctx, stream, 4);
  return hipSuccess;
}

hipError_t launch_shamap_tree_report(const TreeGen& g, uint8_t* root, uint32_t* counts, hipStream_t stream,
                                     uint32_t* node_count) {
  if (!root || ((uintptr_t)root & 3u) || ((uintptr_t)counts & 3u) || ((uintptr_t)node_count & 3u))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(tree_finish_kernel, dim3(1), dim3(64), 0, stream, g.meta, static_cast<const uint32_t*>(nullptr), 0u,
                     reinterpret_cast<uint32_t*>(root), counts, static_cast<const uint32_t*>(nullptr), node_count);
  return hipGetLastError();
}

hipError_t launch_shamap_tree_snapshot(const TreeGen& from, uint32_t from_capacity, uint32_t items_bound,
                                       const TreeGen& to, uint32_t capacity, uint8_t* root, uint32_t* counts,
                                       uint32_t* node_count, bool (*fault)(), hipStream_t stream) {
  if (!root || ((uintptr_t)root & 3u) || ((uintptr_t)counts & 3u) || ((uintptr_t)node_count & 3u))
    return hipErrorInvalidValue;
  if (capacity == 0 || from_capacity == 0 || items_bound > from_capacity || items_bound > capacity)
    return hipErrorInvalidValue;
  const uint32_t units = 2 * items_bound > kSnapFixedUnits ? 2 * items_bound : kSnapFixedUnits;
  TR_LAUNCH(tree_snapshot_kernel, grid_of(units), kTrBlock, from, from_capacity, to, capacity);
  const uint32_t* const no_words = nullptr;
  TR_LAUNCH(tree_finish_kernel, 1, 64, to.meta, no_words, 0u, reinterpret_cast<uint32_t*>(root), counts, no_words,
            node_count);
  return hipSuccess;
}

hipError_t launch_shamap_tree_export(const TreeGen& g, uint32_t items_bound, uint8_t* key, uint8_t* leaf,
                                     uint32_t rows, uint32_t* items, hipStream_t stream) {
  if (items_bound > rows || ((uintptr_t)key & 15u) || ((uintptr_t)leaf & 15u) || ((uintptr_t)items & 3u))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(tree_export_kernel, dim3(grid_of(items_bound ? items_bound : 1)), dim3(kTrBlock), 0, stream, g.key,
                     g.leaf, g.meta, rows, key, leaf, items);
  return hipGetLastError();
}

}  // namespace stl
