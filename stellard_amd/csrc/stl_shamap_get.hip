// stl_shamap_get.hip -- gfx950 kernels of a resident SHAMap's answers by node ID
// (stl_shamap_tree_get_nodes*: getNodeFat and getPath; stl_shamap_get_core.h has
// the rules).  Nothing here writes a tree: every array written is the caller's
// or the stream context's.
//
// One call, all on the caller's stream:
//   1. ranges    the bucket counts are scanned into begin positions; one lane
//                per request finds its range (a bisection of its bucket at
//                depth >= 4, two begins above), applies the rules and writes
//                status, rows, leaf key and leaf hash; rows is scanned into first
//   2. tasks     one lane per request lists its rows again and writes, for every
//                row below max_nodes, the task (depth, position of the node's
//                first key) at the row's own index, and marks the bucket of
//                every task at depth >= 4
//   3. gather    the marked buckets' keys and leaf hashes go into one scratch,
//                in order; the neighbour kernel of stl_shamap.hip runs over it
//   4. levels    depth 63 down to 4: get_rows_kernel, then the plain level
//                kernel.  Just before level d runs, the slots of a depth-d
//                node's branches hold its children's hashes and the slot of a
//                depth-(d + 1) node's first key holds that node's hash, so each
//                task of depth d gathers its node's body there (16 lanes, one
//                per branch) and each task of depth d + 1 takes its hash.
//                Nothing is hashed twice, and a node that several rows want is
//                stored by each of them: no sort of the tasks, no search per
//                node, no copy pass, and the level kernel is stl_shamap.hip's own.
//   5. top       up to four launches fold the bucket values into the 4,369
//                prefixes above them (only the depths a task reads); one launch
//                stores the rows of the tasks at depth < 4 from those values
//   6. finish    the count and the eight counts -- the only launch that writes
//                the caller's count words
//
// Every count is read on the device; the grids come from n, the task rows and
// the host's bound of the item count.  Every read of the generation is clamped
// by its count and capacity, every read of the scratch by the rows gathered,
// every store into the caller's node arrays by max_nodes.
#include "stl_shamap_get.h"

#include "stl_shamap.h"
#include "stl_shamap_fetch_core.h"
#include "stl_shamap_get_core.h"

namespace stl {

namespace {

constexpr uint32_t kGnBlock = 256;  // 4 waves per workgroup
constexpr uint32_t kGnGroup = 16;   // lanes per task: one per branch
constexpr uint32_t kGnTasksPerBlock = kGnBlock / kGnGroup;
constexpr uint32_t kGnRowsGrid = 1024;
constexpr uint32_t kGnNone = 0xffffffffu;
// header words of the workspace
constexpr uint32_t kGhTotal = 0, kGhInner = 1, kGhLeaf = 2, kGhOther = 3, kGhBuckets = 4, kGhDistinct = 5;
constexpr uint32_t kGhTopNeed = 6, kGhWords = 64;  // [6]: 4 - the shallowest depth of a task above the buckets
// a tree's top values: the prefixes of length 3, 2, 1 and the root, one after another
constexpr uint32_t kGnTopValues = kTreeTopValues + 1;

__device__ __forceinline__ void gn_st8(uint8_t* p, size_t row, const uint32_t k[8]) {
  uint4* q = reinterpret_cast<uint4*>(p + 32 * row);
  q[0] = make_uint4(k[0], k[1], k[2], k[3]);
  q[1] = make_uint4(k[4], k[5], k[6], k[7]);
}

__device__ __forceinline__ void gn_count(bool v, uint32_t* word) {
  const uint64_t b = __ballot(v);
  if ((threadIdx.x & 63u) == 0 && b != 0) atomicAdd(word, (uint32_t)__popcll(b));
}

// The bucket of the key at row pos, from its first two bytes.
__device__ __forceinline__ uint32_t gn_bucket_at(const uint8_t* __restrict__ key, uint32_t pos) {
  const uint32_t w = *reinterpret_cast<const uint32_t*>(key + 32 * (size_t)pos);
  return ((w & 0xffu) << 8) | ((w >> 8) & 0xffu);
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
uint32_t grid_of(uint32_t n) { return (n + kGnBlock - 1) / kGnBlock; }

// The workspace's parts, in order.  The header, the scratch header, the marks
// and the top's seen words lie side by side: one memset clears them.
struct GetWs {
  uint32_t *gh, *hdr, *mark, *seen_top, *begin, *sz, *off, *topcnt, *toph, *task_pos;
  uint8_t* task_depth;
  int8_t* l;
  uint8_t *skey, *slot;
  unsigned long long* seen;
  void* temp;
  size_t bytes, clear_bytes;
  GetWs(void* base, size_t bound, size_t tasks, size_t temp_bytes) {
    uint8_t* p = static_cast<uint8_t*>(base);
    size_t o = 0;
    auto take = [&](size_t b) {
      uint8_t* q = p + o;
      o += up256(b);
      return q;
    };
    auto words = [&](size_t n) { return reinterpret_cast<uint32_t*>(take(4 * n)); };
    gh = words(kGhWords);
    hdr = reinterpret_cast<uint32_t*>(take(kShamapHeaderBytes));
    mark = words(kTreeBuckets);
    seen_top = words(kGnTopValues);
    clear_bytes = o;
    begin = words(kTreeBuckets);
    sz = words(kTreeBuckets);
    off = words(kTreeBuckets);
    topcnt = words(kGnTopValues);
    toph = words(8 * kGnTopValues);
    task_pos = words(tasks);
    task_depth = take(tasks);
    l = reinterpret_cast<int8_t*>(take(bound));
    skey = take(32 * bound);
    slot = take(32 * bound);
    seen = reinterpret_cast<unsigned long long*>(take(8 * bound));
    temp = p + o;
    bytes = o + up256(temp_bytes);
  }
};

// What the kernels read of the generation.
struct GetGen {
  const uint8_t* key;
  const uint8_t* leaf;
  const uint32_t* bcnt;
  const uint32_t* bh;
  const uint32_t* meta;
  uint32_t cap;
};

__device__ __forceinline__ GetTree gn_tree(const GetGen& g, const uint32_t* begin) {
  return GetTree{g.key, begin, g.bcnt, shamap_tree_readable(g.meta[0], g.cap)};
}

// 1. one lane per request: status, rows, the leaf.
__global__ __launch_bounds__(kGnBlock) void get_plan_kernel(GetGen g, const uint32_t* __restrict__ begin, ShamapGet rq,
                                                            uint32_t n, uint32_t* gh) {
  const uint32_t i = blockIdx.x * kGnBlock + threadIdx.x;
  uint32_t st = kGnNone;
  if (i < n) {
    const GetTree t = gn_tree(g, begin);
    uint32_t id[8], rows = 0, leaf_pos = kGetNoLeaf;
    shamap_load_key(id, rq.id, i);
    const uint32_t mode = rq.mode ? rq.mode[i] : kGetFat;
    st = shamap_get_request(t, id, rq.depth[i], mode, false, [](uint32_t, uint32_t, uint32_t) {}, &rows, &leaf_pos);
    rq.status[i] = (uint8_t)st;
    rq.rows[i] = rows;
    uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool leaf = leaf_pos < t.m;
    if (rq.leaf_key) {
      if (leaf) shamap_load_key(v, g.key, leaf_pos);
      gn_st8(rq.leaf_key, i, v);
    }
    if (rq.leaf_hash) {
      if (leaf) shamap_load_key(v, g.leaf, leaf_pos);
      gn_st8(rq.leaf_hash, i, v);
    }
  }
  gn_count(st == kAtInner, &gh[kGhInner]);
  gn_count(st == kAtLeaf || st == kAtOtherLeaf, &gh[kGhLeaf]);
  gn_count(st == kAtAbsent || st == kAtEmptyRoot || st == kAtInvalid, &gh[kGhOther]);
}

// 2. one lane per request: its rows' tasks, at the rows' own indices below
// `tasks`, and the marks.  The last request states the total.
__global__ __launch_bounds__(kGnBlock) void get_tasks_kernel(GetGen g, const uint32_t* __restrict__ begin, ShamapGet rq,
                                                             uint32_t n, uint32_t tasks,
                                                             uint32_t* __restrict__ task_pos,
                                                             uint8_t* __restrict__ task_depth,
                                                             uint32_t* __restrict__ mark, uint32_t* gh) {
  const uint32_t i = blockIdx.x * kGnBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t first = rq.first[i], want = rq.rows[i];
  if (i == n - 1) gh[kGhTotal] = first + want;
  if (want == 0 || first >= tasks) return;
  const GetTree t = gn_tree(g, begin);
  uint32_t id[8], rows = 0, leaf_pos = kGetNoLeaf;
  shamap_load_key(id, rq.id, i);
  const uint32_t mode = rq.mode ? rq.mode[i] : kGetFat;
  shamap_get_request(
      t, id, rq.depth[i], mode, true,
      [&](uint32_t j, uint32_t d, uint32_t pos) {
        const uint32_t r = first + j;
        if (j >= want || r >= tasks) return;
        task_pos[r] = pos;
        task_depth[r] = (uint8_t)d;
        if (d >= kTreeBucketDepth && pos < t.m) mark[gn_bucket_at(g.key, pos)] = 1u;
        if (d < kTreeBucketDepth) atomicMax(&gh[kGhTopNeed], kTreeBucketDepth - d);  // the folds this row needs
      },
      &rows, &leaf_pos);
}

// 3a. kTreeBuckets lanes exactly: a marked bucket sends all its keys.
__global__ __launch_bounds__(kGnBlock) void get_buckets_kernel(const uint32_t* __restrict__ bcnt,
                                                               const uint32_t* __restrict__ mark,
                                                               uint32_t* __restrict__ sz, uint32_t* gh) {
  const uint32_t b = blockIdx.x * kGnBlock + threadIdx.x;
  const bool marked = mark[b] != 0;
  sz[b] = marked ? bcnt[b] : 0u;
  gn_count(marked, &gh[kGhBuckets]);
}

// 3b. scratch row p <- the row of its bucket in the generation, and a clear
// seen word.  rows: what the scratch was sized for.  The first lane states the total.
__global__ __launch_bounds__(kGnBlock) void get_gather_kernel(GetGen g, const uint32_t* __restrict__ begin,
                                                              const uint32_t* __restrict__ sz,
                                                              const uint32_t* __restrict__ off, uint32_t rows,
                                                              uint32_t* __restrict__ hdr, uint8_t* __restrict__ skey,
                                                              uint8_t* __restrict__ slot,
                                                              unsigned long long* __restrict__ seen) {
  const uint32_t p = blockIdx.x * kGnBlock + threadIdx.x;
  uint32_t total = off[kTreeBuckets - 1] + sz[kTreeBuckets - 1];
  if (total > rows) total = rows;  // never: no more keys are gathered than the tree holds
  if (p == 0) hdr[kShamapHdrDistinct] = total;
  if (p >= total) return;
  const uint32_t m = shamap_tree_readable(g.meta[0], g.cap);
  const uint32_t b = shamap_diff_bucket_of(off, p);
  uint32_t lo, hi;
  shamap_lookup_range(begin[b], g.bcnt[b], m, &lo, &hi);
  const uint32_t src = lo + (p - off[b]);
  uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (src < hi) shamap_load_key(v, g.key, src);  // always, while the counts describe the keys
  gn_st8(skey, p, v);
  if (src < hi) shamap_load_key(v, g.leaf, src);
  gn_st8(slot, p, v);
  seen[p] = 0ull;
}

// Where the rows go (ShamapEmit's arrays) and the tasks that name them.
struct GetEmit {
  uint8_t* hash;
  uint8_t* body;
  uint8_t* id;
  uint32_t* meta;
  uint32_t max_nodes;
  const uint32_t* task_pos;
  const uint8_t* task_depth;
  uint32_t tasks;
  uint32_t* gh;
};

__device__ __forceinline__ uint32_t gn_task_count(const GetEmit& em) {
  uint32_t t = em.gh[kGhTotal];
  if (t > em.max_nodes) t = em.max_nodes;
  return t < em.tasks ? t : em.tasks;
}

// The scratch position of task r's node, or kGnNone: its bucket's place in the
// scratch plus the key's place in its bucket.
__device__ __forceinline__ uint32_t gn_task_at(const GetGen& g, const uint32_t* __restrict__ begin,
                                               const uint32_t* __restrict__ mark, const uint32_t* __restrict__ off,
                                               uint32_t pos, uint32_t m, uint32_t ms) {
  if (pos >= m) return kGnNone;
  const uint32_t b = gn_bucket_at(g.key, pos);
  const uint32_t bb = begin[b];
  if (!mark[b] || pos < bb) return kGnNone;
  const uint32_t a = shamap_get_scratch_pos(pos, bb, off[b]);
  return a < ms ? a : kGnNone;  // always below: a marked bucket is gathered whole
}

// 4. Between the level launches of depth d + 1 and depth d (d = 63 .. 3; no
// level runs above 63 or below 4).  Just now the slots of a depth-d node's
// branches hold its children's hashes, and the slot of a depth-(d + 1) node's
// first key holds that node's own hash.  So, 16 lanes a task and one per branch:
// a task of depth d gathers its node's body, ID and leaf mask into its row, and
// a task of depth d + 1 takes its row's hash.  Nothing is hashed here -- the
// level kernel does that once per node, whoever asks.
__global__ __launch_bounds__(kGnBlock) void get_rows_kernel(GetGen g, const uint32_t* __restrict__ begin,
                                                            const uint32_t* __restrict__ mark,
                                                            const uint32_t* __restrict__ off,
                                                            const uint32_t* __restrict__ hdr,
                                                            const int8_t* __restrict__ l,
                                                            const uint8_t* __restrict__ skey,
                                                            const uint8_t* __restrict__ slot,
                                                            unsigned long long* seen, uint32_t d, GetEmit em) {
  const bool bodies = d >= kTreeBucketDepth && hdr[d] != 0, hashes = d + 1 < kShamapDepths && hdr[d + 1] != 0;
  if (!bodies && !hashes) return;  // uniform: the scratch holds no node at either depth
  const uint32_t T = gn_task_count(em);
  const uint32_t ms = hdr[kShamapHdrDistinct];
  const uint32_t m = shamap_tree_readable(g.meta[0], g.cap);
  const uint32_t tid = threadIdx.x, grp = tid / kGnGroup, c = tid % kGnGroup;
  for (uint32_t base = blockIdx.x * kGnTasksPerBlock; base < T; base += gridDim.x * kGnTasksPerBlock) {  // uniform
    const uint32_t r = base + grp;
    const uint32_t td = r < T ? em.task_depth[r] : kGnNone;
    uint32_t a = kGnNone;
    if ((bodies && td == d) || (hashes && td == d + 1)) a = gn_task_at(g, begin, mark, off, em.task_pos[r], m, ms);
    if (a != kGnNone && td == d + 1 && c < 2 && r < em.max_nodes) {  // the hash, 16 bytes a lane
      const uint4* q = reinterpret_cast<const uint4*>(slot + 32 * (size_t)a);
      reinterpret_cast<uint4*>(em.hash + 32 * (size_t)r)[c] = q[c];
    }
    bool leaf = false;
    const bool body = a != kGnNone && td == d;
    if (body) {
      const uint32_t e = shamap_range_end(skey, ms, a, d);
      const uint32_t p = shamap_branch_first(skey, a, e, d, c);
      uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0;
      if (p < e) {
        const uint4* q = reinterpret_cast<const uint4*>(slot + 32 * (size_t)p);
        h0 = q[0];
        h1 = q[1];
        leaf = shamap_branch_is_leaf(l, p, e, d);
      }
      if (r < em.max_nodes) {  // always: T <= max_nodes
        uint4* q = reinterpret_cast<uint4*>(em.body + 512 * (size_t)r + 32 * c);
        q[0] = h0;
        q[1] = h1;
      }
    }
    // a task's 16 lanes sit side by side in their wave
    const uint64_t leaves = __ballot(leaf);
    if (body && c == 0) {
      if (r < em.max_nodes) {
        if (em.id) {
          uint32_t key[8], id[8];
          shamap_load_key(key, skey, a);
          shamap_mask_key(id, key, d);
          gn_st8(em.id, r, id);
        }
        if (em.meta) em.meta[r] = shamap_node_meta(d, (uint32_t)(leaves >> (tid & 48u)) & 0xffffu);
      }
      const unsigned long long bit = 1ull << d;
      if (!(atomicOr(&seen[a], bit) & bit)) atomicAdd(&em.gh[kGhDistinct], 1u);
    }
  }
}

// 5a. one depth of the top: `nodes` prefixes of length `depth` from 16 children
// each, 64 to a workgroup of one wave.  A lane's record is 129 dwords from the
// next, so the wave hashes out of 64 different banks.
__global__ __launch_bounds__(64) void get_top_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ h,
                                                     uint32_t nodes, uint32_t depth, uint32_t* __restrict__ out_cnt,
                                                     uint32_t* __restrict__ out_h, const uint32_t* __restrict__ gh) {
  __shared__ uint32_t recs[64 * kShamapRecordWords];
  // uniform: a task of depth d reads the values of depths d and d + 1, so the
  // fold of `depth` serves the tasks at that depth or above it
  if (gh[kGhTopNeed] < kTreeBucketDepth - depth) return;
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= nodes) return;
  uint32_t v[8];
  uint32_t* const rec = recs + threadIdx.x * kShamapRecordWords;
  out_cnt[t] = shamap_fetch_top_value(cnt + 16 * t, h + 128 * (size_t)t, depth == 0, rec, v);
  for (uint32_t i = 0; i < 8; ++i) out_h[8 * t + i] = v[i];
}

// 5b. The rows of the tasks at depth < 4, from the folded values: 16 lanes a
// task, one per branch; the node's hash is its prefix's value.
__global__ __launch_bounds__(kGnBlock) void get_top_rows_kernel(GetGen g, const uint32_t* __restrict__ topcnt,
                                                                const uint32_t* __restrict__ toph,
                                                                uint32_t* seen_top, GetEmit em) {
  const uint32_t T = gn_task_count(em);
  const uint32_t m = shamap_tree_readable(g.meta[0], g.cap);
  const uint32_t tid = threadIdx.x, grp = tid / kGnGroup, c = tid % kGnGroup;
  for (uint32_t base = blockIdx.x * kGnTasksPerBlock; base < T; base += gridDim.x * kGnTasksPerBlock) {  // uniform
    const uint32_t r = base + grp;
    uint32_t d = kGnNone, pos = 0;
    if (r < T && em.task_depth[r] < kTreeBucketDepth) {
      pos = em.task_pos[r];
      if (pos < m) d = em.task_depth[r];
    }
    bool leaf = false;
    uint32_t t = 0;
    if (d != kGnNone) {
      t = d ? gn_bucket_at(g.key, pos) >> (4u * (kTreeBucketDepth - d)) : 0u;
      const uint32_t child = 16u * t + c;
      const uint32_t* ccnt = d == 3u ? g.bcnt + child : topcnt + shamap_get_top_index(d + 1u, child);
      const uint32_t* ch = d == 3u ? g.bh + 8 * (size_t)child : toph + 8 * (size_t)shamap_get_top_index(d + 1u, child);
      const uint32_t cc = *ccnt;
      uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0;
      if (cc) {
        h0 = reinterpret_cast<const uint4*>(ch)[0];
        h1 = reinterpret_cast<const uint4*>(ch)[1];
      }
      leaf = cc == 1u;
      if (r < em.max_nodes) {  // always: T <= max_nodes
        uint4* q = reinterpret_cast<uint4*>(em.body + 512 * (size_t)r + 32 * c);
        q[0] = h0;
        q[1] = h1;
      }
    }
    const uint64_t leaves = __ballot(leaf);
    if (d != kGnNone && c == 0) {
      const uint32_t own = shamap_get_top_index(d, t);
      if (r < em.max_nodes) {
        uint32_t v[8], key[8], id[8];
        shamap_load_key(v, reinterpret_cast<const uint8_t*>(toph), own);
        gn_st8(em.hash, r, v);
        if (em.id) {
          shamap_load_key(key, g.key, pos);
          shamap_mask_key(id, key, d);
          gn_st8(em.id, r, id);
        }
        if (em.meta) em.meta[r] = shamap_node_meta(d, (uint32_t)(leaves >> (tid & 48u)) & 0xffffu);
      }
      if (atomicExch(&seen_top[own], 1u) == 0u) atomicAdd(&em.gh[kGhDistinct], 1u);
    }
  }
}

// 6. the count and the eight counts.
__global__ __launch_bounds__(64) void get_finish_kernel(const uint32_t* __restrict__ gh,
                                                        const uint32_t* __restrict__ hdr,
                                                        const uint32_t* __restrict__ meta, uint32_t cap,
                                                        uint32_t* __restrict__ count, uint32_t* __restrict__ counts) {
  if (threadIdx.x != 0) return;
  *count = gh[kGhTotal];
  if (!counts) return;
  counts[0] = gh[kGhTotal];
  counts[1] = gh[kGhInner];
  counts[2] = gh[kGhLeaf];
  counts[3] = gh[kGhOther];
  counts[4] = gh[kGhBuckets];
  counts[5] = hdr[kShamapHdrDistinct];
  counts[6] = gh[kGhDistinct];
  counts[7] = shamap_tree_readable(meta[0], cap);
}

}  // namespace

uint32_t shamap_get_task_rows(size_t n, uint32_t max_nodes) {
  const uint64_t most = (uint64_t)n * kGetMaxRows;
  return most < max_nodes ? (uint32_t)most : max_nodes;
}

size_t shamap_get_workspace_bytes(size_t bound, size_t tasks, size_t temp_bytes) {
  return GetWs(nullptr, bound, tasks, temp_bytes).bytes;
}

#define GN_TRY(expr)                              \
  do {                                            \
    if (fault && fault()) return hipErrorUnknown; \
    const hipError_t e_ = (expr);                 \
    if (e_ != hipSuccess) return e_;              \
  } while (0)

#define GN_LAUNCH(kernel, grid, block, ...)                                      \
  do {                                                                           \
    if (fault && fault()) return hipErrorUnknown;                                \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
    const hipError_t e_ = hipGetLastError();                                     \
    if (e_ != hipSuccess) return e_;                                             \
  } while (0)

#define GN_RC(expr)                  \
  do {                               \
    const hipError_t e_ = (expr);    \
    if (e_ != hipSuccess) return e_; \
  } while (0)

hipError_t launch_shamap_tree_get_nodes(const TreeGen& gen, uint32_t cap, uint32_t bound, const ShamapGet& rq,
                                        uint32_t n, const ShamapEmit& emit, uint32_t* counts, void* ws,
                                        size_t temp_bytes, bool (*fault)(), const PhaseClock* clock,
                                        hipStream_t stream) {
  if (!ws || ((uintptr_t)ws & 255u) || cap == 0 || bound > cap || n == 0) return hipErrorInvalidValue;
  if (!rq.id || !rq.depth || !rq.status || !rq.first || !rq.rows) return hipErrorInvalidValue;
  if (!emit.hash || !emit.body || !emit.count) return hipErrorInvalidValue;
  if ((((uintptr_t)emit.hash | (uintptr_t)emit.body | (uintptr_t)emit.id | (uintptr_t)rq.id | (uintptr_t)rq.leaf_key |
        (uintptr_t)rq.leaf_hash) & 15u) ||
      (((uintptr_t)emit.meta | (uintptr_t)emit.count | (uintptr_t)counts | (uintptr_t)rq.first | (uintptr_t)rq.rows) &
       3u))
    return hipErrorInvalidValue;
  const uint32_t tasks = shamap_get_task_rows(n, emit.max_nodes);
  const GetWs w(ws, bound, tasks, temp_bytes);
  const GetGen g{gen.key, gen.leaf, gen.bcnt, gen.bh, gen.meta, cap};
  const GetEmit em{emit.hash, emit.body, emit.id, emit.meta, emit.max_nodes, w.task_pos, w.task_depth, tasks, w.gh};
  const uint32_t gb = kTreeBuckets / kGnBlock;
  const bool stores = tasks != 0, gathers = stores && bound != 0;
  uint32_t rows_grid = (tasks + kGnTasksPerBlock - 1) / kGnTasksPerBlock;
  if (rows_grid > kGnRowsGrid) rows_grid = kGnRowsGrid;
  if (clock) clock->mark(clock->ctx, stream, 0);
  GN_TRY(hipMemsetAsync(w.gh, 0, w.clear_bytes, stream));
  // 1. ranges
  GN_RC(shamap_exclusive_scan(w.temp, temp_bytes, gen.bcnt, w.begin, kTreeBuckets, fault, stream));
  GN_LAUNCH(get_plan_kernel, grid_of(n), kGnBlock, g, w.begin, rq, n, w.gh);
  GN_RC(shamap_exclusive_scan(w.temp, temp_bytes, rq.rows, rq.first, n, fault, stream));
  // 2. tasks
  GN_LAUNCH(get_tasks_kernel, grid_of(n), kGnBlock, g, w.begin, rq, n, tasks, w.task_pos, w.task_depth, w.mark, w.gh);
  if (gathers) {
    // 3. gather
    GN_LAUNCH(get_buckets_kernel, gb, kGnBlock, gen.bcnt, w.mark, w.sz, w.gh);
    GN_RC(shamap_exclusive_scan(w.temp, temp_bytes, w.sz, w.off, kTreeBuckets, fault, stream));
    GN_LAUNCH(get_gather_kernel, grid_of(bound), kGnBlock, g, w.begin, w.sz, w.off, bound, w.hdr, w.skey, w.slot,
              w.seen);
    GN_RC(launch_shamap_neighbours(w.hdr, w.l, w.skey, bound, fault, stream));
  }
  if (clock) clock->mark(clock->ctx, stream, 1);
  if (gathers) {
    // 4. levels: the bodies of depth d and the hashes of depth d + 1 just before depth d is hashed
    for (int d = (int)kShamapDepths - 1; d >= (int)kTreeBucketDepth - 1; --d) {
      GN_LAUNCH(get_rows_kernel, rows_grid, kGnBlock, g, w.begin, w.mark, w.off, w.hdr, w.l, w.skey, w.slot, w.seen,
                (uint32_t)d, em);
      if (d >= (int)kTreeBucketDepth)
        GN_RC(launch_shamap_level(w.hdr, w.l, w.skey, w.slot, bound, (uint32_t)d, fault, stream));
    }
  }
  if (clock) clock->mark(clock->ctx, stream, 2);
  if (stores) {
    // 5. top: the prefixes of length 3, 2, 1 and the root, then their rows
    const uint32_t *c = gen.bcnt, *h = gen.bh;
    uint32_t o = 0;
    for (uint32_t depth = kTreeBucketDepth; depth-- > 0;) {
      const uint32_t nodes = 1u << (4 * depth);
      GN_LAUNCH(get_top_kernel, (nodes + 63) / 64, 64, c, h, nodes, depth, w.topcnt + o, w.toph + 8 * o, w.gh);
      c = w.topcnt + o, h = w.toph + 8 * o;
      o += nodes;
    }
    GN_LAUNCH(get_top_rows_kernel, rows_grid, kGnBlock, g, w.topcnt, w.toph, w.seen_top, em);
  }
  // 6. finish
  GN_LAUNCH(get_finish_kernel, 1, 64, w.gh, w.hdr, gen.meta, cap, emit.count, counts);
  if (clock) {
    clock->mark(clock->ctx, stream, 3);
    clock->mark(clock->ctx, stream, 4);
  }
  return hipSuccess;
}

}  // namespace stl
