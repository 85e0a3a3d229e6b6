// stl_shamap_lookup.hip -- gfx950 kernels of the resident SHAMap's read-only
// calls (stl_shamap_lookup_core.h has the rules).  Nothing here writes a tree.
//
// Lookup (stl_shamap_tree_lookup*), on the caller's stream:
//   1. begin     the live generation's 65,536 bucket counts are scanned
//   2. lookup    one lane per query: its bucket from the key's first four
//                nibbles, a bisection of that bucket's range alone; the found
//                bits go out by one ballot per wave, whole words, no atomics
//
// Compare (stl_shamap_tree_compare*), on the caller's stream:
//   1. buckets   65,536 lanes compare the two generations' bucket values; a
//                bucket that differs gets cnt_a + cnt_b slots, an equal one none;
//                the two count arrays and the slot counts are scanned
//   2. slots     one lane per slot: the item (of a, then of b) bisects the other
//                tree's range of the same bucket and writes its flag and source
//                rows at its merged rank -- every slot once, in key order
//   3. rows      the flags are scanned; one lane per slot copies a difference's
//                key, kind and leaf hashes to its row when that is below max_rows
//   4. finish    the eight counts -- the only launch that writes them
//
// Every count is read on the device; the grids come from host-known bounds.
// Every read of a generation is guarded by its item count (clamped to the
// capacity), every store into the workspace by the slots it was sized for and
// every store into the caller's rows by max_rows.
#include "stl_shamap_lookup.h"

#include "stl_shamap.h"
#include "stl_shamap_lookup_core.h"

namespace stl {

namespace {

constexpr uint32_t kLkBlock = 256;
// header words of a compare's workspace
constexpr uint32_t kDhAOnly = 0, kDhBOnly = 1, kDhChanged = 2, kDhBuckets = 3, kDhWords = 64;

__device__ __forceinline__ void lk_st8(uint8_t* p, size_t row, const uint32_t k[8]) {
  uint4* q = reinterpret_cast<uint4*>(p + 32 * row);
  q[0] = make_uint4(k[0], k[1], k[2], k[3]);
  q[1] = make_uint4(k[4], k[5], k[6], k[7]);
}

__device__ __forceinline__ void lk_count(bool v, uint32_t* word) {
  const uint64_t b = __ballot(v);
  if ((threadIdx.x & 63u) == 0 && b != 0) atomicAdd(word, (uint32_t)__popcll(b));
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
uint32_t grid_of(uint32_t n) { return (n + kLkBlock - 1) / kLkBlock; }

struct LookupWs {
  uint32_t* begin;
  void* temp;
  size_t bytes;
  LookupWs(void* base, size_t temp_bytes) {
    uint8_t* p = static_cast<uint8_t*>(base);
    begin = reinterpret_cast<uint32_t*>(p);
    size_t o = up256(4 * kTreeBuckets);
    temp = p + o;
    bytes = o + up256(temp_bytes);
  }
};

struct CompareWs {
  uint32_t *hdr, *begin_a, *begin_b, *sz, *off, *flag, *scan, *row_a, *row_b;
  void* temp;
  size_t bytes;
  CompareWs(void* base, size_t slots, size_t temp_bytes) {
    uint8_t* p = static_cast<uint8_t*>(base);
    size_t o = 0;
    auto take = [&](size_t b) {
      uint32_t* q = reinterpret_cast<uint32_t*>(p + o);
      o += up256(b);
      return q;
    };
    hdr = take(4 * kDhWords);
    begin_a = take(4 * kTreeBuckets);
    begin_b = take(4 * kTreeBuckets);
    sz = take(4 * kTreeBuckets);
    off = take(4 * kTreeBuckets);
    flag = take(4 * slots);
    scan = take(4 * slots);
    row_a = take(4 * slots);
    row_b = take(4 * slots);
    temp = p + o;
    bytes = o + up256(temp_bytes);
  }
};

// Lookup 2.  kBuckets = false: the whole array is bisected (the A/B variant).
template <bool kBuckets>
__global__ __launch_bounds__(kLkBlock) void tree_lookup_kernel(
    const uint8_t* __restrict__ rkey, const uint8_t* __restrict__ rleaf, const uint32_t* __restrict__ bcnt,
    const uint32_t* __restrict__ begin, const uint32_t* __restrict__ meta, uint32_t cap,
    const uint8_t* __restrict__ qkey, uint32_t n, uint64_t* __restrict__ words, uint8_t* __restrict__ leaf,
    uint32_t* __restrict__ position) {
  const uint32_t i = blockIdx.x * kLkBlock + threadIdx.x;
  const uint32_t m = meta[0] < cap ? meta[0] : cap;
  bool found = false;
  if (i < n) {
    uint32_t key[8], v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    shamap_load_key(key, qkey, i);
    uint32_t lo = 0, hi = m;
    if constexpr (kBuckets) {
      const uint32_t b = shamap_tree_bucket(key);
      shamap_lookup_range(begin[b], bcnt[b], m, &lo, &hi);
    }
    const uint32_t p = shamap_lookup_lower_bound(rkey, lo, hi, key, &found);
    if (leaf) {
      if (found) shamap_load_key(v, rleaf, p);
      lk_st8(leaf, i, v);
    }
    if (position) position[i] = found ? p : kDiffNoRow;
  }
  // the wave's 64 rows are one word; rows past n are clear bits of the last word
  const uint64_t bits = __ballot(found);
  if ((threadIdx.x & 63u) == 0 && i < n) words[i >> 6] = bits;
}

// Compare 1.  kTreeBuckets lanes exactly.
__global__ __launch_bounds__(kLkBlock) void tree_diff_buckets_kernel(const uint32_t* __restrict__ cnt_a,
                                                                     const uint32_t* __restrict__ h_a,
                                                                     const uint32_t* __restrict__ cnt_b,
                                                                     const uint32_t* __restrict__ h_b,
                                                                     uint32_t* __restrict__ sz, uint32_t* hdr) {
  const uint32_t b = blockIdx.x * kLkBlock + threadIdx.x;
  uint32_t x[8], y[8];
  shamap_load_key(x, reinterpret_cast<const uint8_t*>(h_a), b);
  shamap_load_key(y, reinterpret_cast<const uint8_t*>(h_b), b);
  const uint32_t ca = cnt_a[b], cb = cnt_b[b];
  const bool differs = shamap_bucket_differs(ca, x, cb, y);
  sz[b] = differs ? ca + cb : 0u;
  lk_count(differs, &hdr[kDhBuckets]);
}

// The slots of the buckets that differ, never above what the workspace holds.
__device__ __forceinline__ uint32_t diff_total(const uint32_t* __restrict__ sz, const uint32_t* __restrict__ off,
                                               uint32_t slots) {
  const uint32_t t = off[kTreeBuckets - 1] + sz[kTreeBuckets - 1];
  return t < slots ? t : slots;
}

// Compare 2.
__global__ __launch_bounds__(kLkBlock) void tree_diff_slots_kernel(
    const uint8_t* __restrict__ ka, const uint8_t* __restrict__ la, const uint32_t* __restrict__ cnt_a,
    const uint32_t* __restrict__ begin_a, const uint32_t* __restrict__ meta_a, uint32_t cap_a,
    const uint8_t* __restrict__ kb, const uint8_t* __restrict__ lb, const uint32_t* __restrict__ cnt_b,
    const uint32_t* __restrict__ begin_b, const uint32_t* __restrict__ meta_b, uint32_t cap_b,
    const uint32_t* __restrict__ sz, const uint32_t* __restrict__ off, uint32_t slots, uint32_t* __restrict__ flag,
    uint32_t* __restrict__ row_a, uint32_t* __restrict__ row_b, uint32_t* hdr) {
  const uint32_t p = blockIdx.x * kLkBlock + threadIdx.x;
  const uint32_t total = diff_total(sz, off, slots);
  uint32_t kind = kDiffNone;
  if (p < total) {
    const uint32_t ma = meta_a[0] < cap_a ? meta_a[0] : cap_a;
    const uint32_t mb = meta_b[0] < cap_b ? meta_b[0] : cap_b;
    const uint32_t b = shamap_diff_bucket_of(off, p);
    const uint32_t q = p - off[b];
    uint32_t a0, a1, b0, b1;
    shamap_lookup_range(begin_a[b], cnt_a[b], ma, &a0, &a1);
    shamap_lookup_range(begin_b[b], cnt_b[b], mb, &b0, &b1);
    if (q < (a1 - a0) + (b1 - b0)) {  // always, while the counts describe the keys
      uint32_t ra, rb;
      const uint32_t s = off[b] + shamap_diff_slot(ka, la, a0, a1, kb, lb, b0, b1, q, &kind, &ra, &rb);
      if (s < slots) {
        flag[s] = kind != kDiffNone ? 1u : 0u;
        row_a[s] = ra;
        row_b[s] = rb;
      } else {
        kind = kDiffNone;  // never
      }
    }
  }
  lk_count(kind == kDiffAOnly, &hdr[kDhAOnly]);
  lk_count(kind == kDiffBOnly, &hdr[kDhBOnly]);
  lk_count(kind == kDiffChanged, &hdr[kDhChanged]);
}

// Compare 3.  Slot p that holds a difference -> row scan[p] of the caller's arrays.
__global__ __launch_bounds__(kLkBlock) void tree_diff_rows_kernel(
    const uint8_t* __restrict__ ka, const uint8_t* __restrict__ la, const uint32_t* __restrict__ meta_a, uint32_t cap_a,
    const uint8_t* __restrict__ kb, const uint8_t* __restrict__ lb, const uint32_t* __restrict__ meta_b, uint32_t cap_b,
    const uint32_t* __restrict__ sz, const uint32_t* __restrict__ off, uint32_t slots,
    const uint32_t* __restrict__ flag, const uint32_t* __restrict__ scan, const uint32_t* __restrict__ row_a,
    const uint32_t* __restrict__ row_b, ShamapDiff out) {
  const uint32_t p = blockIdx.x * kLkBlock + threadIdx.x;
  if (p >= diff_total(sz, off, slots) || !flag[p]) return;
  const uint32_t row = scan[p];
  if (row >= out.max_rows) return;
  const uint32_t ma = meta_a[0] < cap_a ? meta_a[0] : cap_a;
  const uint32_t mb = meta_b[0] < cap_b ? meta_b[0] : cap_b;
  const uint32_t ra = row_a[p], rb = row_b[p];
  const bool in_a = ra < ma, in_b = rb < mb;
  if (!in_a && !in_b) return;  // never
  uint32_t v[8];
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (in_a) shamap_load_key(v, ka, ra); else shamap_load_key(v, kb, rb);
  lk_st8(out.key, row, v);
  out.kind[row] = (uint8_t)(in_a ? (in_b ? kDiffChanged : kDiffAOnly) : kDiffBOnly);
  if (out.leaf_a) {
    if (in_a) shamap_load_key(v, la, ra);
    lk_st8(out.leaf_a, row, in_a ? v : zero);
  }
  if (out.leaf_b) {
    if (in_b) shamap_load_key(v, lb, rb);
    lk_st8(out.leaf_b, row, in_b ? v : zero);
  }
}

// Compare 4.  slots = 0: no slot kernel ran (both trees empty by the host's bounds).
__global__ __launch_bounds__(64) void tree_diff_finish_kernel(const uint32_t* __restrict__ meta_a, uint32_t cap_a,
                                                              const uint32_t* __restrict__ meta_b, uint32_t cap_b,
                                                              const uint32_t* __restrict__ sz,
                                                              const uint32_t* __restrict__ off, uint32_t slots,
                                                              const uint32_t* __restrict__ flag,
                                                              const uint32_t* __restrict__ scan,
                                                              const uint32_t* __restrict__ hdr,
                                                              uint32_t* __restrict__ counts) {
  if (threadIdx.x != 0) return;
  const uint32_t total = diff_total(sz, off, slots);
  counts[0] = total ? scan[total - 1] + flag[total - 1] : 0u;
  counts[1] = hdr[kDhAOnly];
  counts[2] = hdr[kDhBOnly];
  counts[3] = hdr[kDhChanged];
  counts[4] = hdr[kDhBuckets];
  counts[5] = total;
  counts[6] = meta_a[0] < cap_a ? meta_a[0] : cap_a;
  counts[7] = meta_b[0] < cap_b ? meta_b[0] : cap_b;
}

}  // namespace

size_t shamap_lookup_workspace_bytes(size_t temp_bytes) { return LookupWs(nullptr, temp_bytes).bytes; }
size_t shamap_compare_workspace_bytes(size_t slots, size_t temp_bytes) {
  return CompareWs(nullptr, slots, temp_bytes).bytes;
}

#define LK_TRY(expr)                              \
  do {                                            \
    if (fault && fault()) return hipErrorUnknown; \
    const hipError_t e_ = (expr);                 \
    if (e_ != hipSuccess) return e_;              \
  } while (0)

#define LK_LAUNCH(kernel, grid, block, ...)                                      \
  do {                                                                           \
    if (fault && fault()) return hipErrorUnknown;                                \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
    const hipError_t e_ = hipGetLastError();                                     \
    if (e_ != hipSuccess) return e_;                                             \
  } while (0)

#define LK_RC(expr)                  \
  do {                               \
    const hipError_t e_ = (expr);    \
    if (e_ != hipSuccess) return e_; \
  } while (0)

hipError_t launch_shamap_tree_lookup(const TreeGen& g, uint32_t capacity, const uint8_t* key, uint32_t n,
                                     uint64_t* words, uint8_t* leaf, uint32_t* position, bool buckets, void* ws,
                                     size_t temp_bytes, bool (*fault)(), hipStream_t stream) {
  if (n == 0 || n > 0xffffffc0u || !key || !words || !ws || capacity == 0) return hipErrorInvalidValue;
  if (((uintptr_t)key & 15u) || ((uintptr_t)leaf & 15u) || ((uintptr_t)words & 7u) || ((uintptr_t)position & 3u) ||
      ((uintptr_t)ws & 255u))
    return hipErrorInvalidValue;
  const LookupWs w(ws, temp_bytes);
  if (buckets) {
    LK_RC(shamap_exclusive_scan(w.temp, temp_bytes, g.bcnt, w.begin, kTreeBuckets, fault, stream));
    LK_LAUNCH(tree_lookup_kernel<true>, grid_of(n), kLkBlock, g.key, g.leaf, g.bcnt, w.begin, g.meta, capacity, key, n,
              words, leaf, position);
  } else {
    LK_LAUNCH(tree_lookup_kernel<false>, grid_of(n), kLkBlock, g.key, g.leaf, g.bcnt, w.begin, g.meta, capacity, key,
              n, words, leaf, position);
  }
  return hipSuccess;
}

hipError_t launch_shamap_tree_compare(const TreeGen& a, uint32_t cap_a, const TreeGen& b, uint32_t cap_b,
                                      uint32_t slots, const ShamapDiff& out, void* ws, size_t temp_bytes,
                                      bool (*fault)(), hipStream_t stream) {
  if (!out.counts || !ws || cap_a == 0 || cap_b == 0 || slots > 2u * 16777216u) return hipErrorInvalidValue;
  if (out.max_rows && (!out.key || !out.kind)) return hipErrorInvalidValue;
  if (((uintptr_t)out.key & 15u) || ((uintptr_t)out.leaf_a & 15u) || ((uintptr_t)out.leaf_b & 15u) ||
      ((uintptr_t)out.counts & 3u) || ((uintptr_t)ws & 255u))
    return hipErrorInvalidValue;
  const CompareWs w(ws, slots, temp_bytes);
  const uint32_t gb = kTreeBuckets / kLkBlock;
  LK_TRY(hipMemsetAsync(w.hdr, 0, 4 * kDhWords, stream));
  // 1. buckets
  LK_LAUNCH(tree_diff_buckets_kernel, gb, kLkBlock, a.bcnt, a.bh, b.bcnt, b.bh, w.sz, w.hdr);
  LK_RC(shamap_exclusive_scan(w.temp, temp_bytes, a.bcnt, w.begin_a, kTreeBuckets, fault, stream));
  LK_RC(shamap_exclusive_scan(w.temp, temp_bytes, b.bcnt, w.begin_b, kTreeBuckets, fault, stream));
  LK_RC(shamap_exclusive_scan(w.temp, temp_bytes, w.sz, w.off, kTreeBuckets, fault, stream));
  if (slots) {
    // 2. slots
    LK_LAUNCH(tree_diff_slots_kernel, grid_of(slots), kLkBlock, a.key, a.leaf, a.bcnt, w.begin_a, a.meta, cap_a, b.key,
              b.leaf, b.bcnt, w.begin_b, b.meta, cap_b, w.sz, w.off, slots, w.flag, w.row_a, w.row_b, w.hdr);
    // 3. rows
    LK_RC(shamap_exclusive_scan(w.temp, temp_bytes, w.flag, w.scan, slots, fault, stream));
    if (out.max_rows)
      LK_LAUNCH(tree_diff_rows_kernel, grid_of(slots), kLkBlock, a.key, a.leaf, a.meta, cap_a, b.key, b.leaf, b.meta,
                cap_b, w.sz, w.off, slots, w.flag, w.scan, w.row_a, w.row_b, out);
  }
  // 4. finish
  LK_LAUNCH(tree_diff_finish_kernel, 1, 64, a.meta, cap_a, b.meta, cap_b, w.sz, w.off, slots, w.flag, w.scan, w.hdr,
            out.counts);
  return hipSuccess;
}

}  // namespace stl
