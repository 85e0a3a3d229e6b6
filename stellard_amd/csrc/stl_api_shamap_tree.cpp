// stl_api_shamap_tree.cpp -- the resident SHAMap (a state tree's root from each
// ledger's changes, the inner nodes an apply makes new, lookup by key, the
// difference of two trees, the fork of one tree into another and the one-step
// revert, the fetch pack against another tree, nodes by node ID and paths by
// key): the stl_shamap_tree_* entry points of include/stl.h; kernels:
// stl_shamap_tree.hip, stl_shamap_lookup.hip, stl_shamap_fetch.hip,
// stl_shamap_get.hip, and the sort and level kernels of stl_shamap.hip.
#include "stl_host.h"
#include "stl_shamap.h"
#include "stl_shamap_fetch.h"
#include "stl_shamap_get.h"
#include "stl_shamap_lookup.h"
#include "stl_shamap_tree.h"
#include "stl_shamap_tree_core.h"

using namespace stl;

// One tree: on one device two generations of (sorted keys, leaf hashes, bucket
// values, count, root) and the work areas of an apply.  `live` names the
// generation that holds the tree; an apply writes the other and the host flips
// `live` once the apply's last enqueue has succeeded, so a failed call leaves
// the tree as it was.  `bound`: the last count the host has read plus the rows
// of every apply since -- never below the count on the device.  A fork writes
// the other generation of its destination from the live one of its source.
struct stl_shamap_tree {
  int ordinal = -1;
  uint32_t capacity = 0;
  int live = 0;
  uint32_t bound = 0;
  // the one-step revert: the other generation is the tree as it was before the
  // last successful apply or fork into it, and prev_bound the bound that went with it
  bool revertible = false;
  uint32_t prev_bound = 0;
  DevBuf rows[2];  // keys, then leaf hashes: 64 B per row of capacity
  DevBuf genfix;   // both generations' bucket values and meta words
  DevBuf fixed, batch, scratch;
  stl::TreeGen gen(int g) const {
    stl::TreeGen o;
    o.key = static_cast<uint8_t*>(rows[g].p);
    o.leaf = o.key + 32 * (size_t)capacity;
    uint8_t* p = static_cast<uint8_t*>(genfix.p) + (size_t)g * stl::shamap_tree_gen_fixed_bytes();
    o.bcnt = reinterpret_cast<uint32_t*>(p);
    o.bh = reinterpret_cast<uint32_t*>(p + align256(4 * stl::kTreeBuckets));
    o.meta = reinterpret_cast<uint32_t*>(p + align256(4 * stl::kTreeBuckets) + align256(32 * stl::kTreeBuckets));
    return o;
  }
  uint64_t bytes() const {
    return (uint64_t)rows[0].cap + rows[1].cap + genfix.cap + fixed.cap + batch.cap + scratch.cap;
  }
  void release() {
    rows[0].release();
    rows[1].release();
    genfix.release();
    fixed.release();
    batch.release();
    scratch.release();
  }
};

namespace {
// Handle first: a handle that is not live is STL_EINVAL on every machine.
LiveSet<stl_shamap_tree, CheckFirst::kHandle> g_trees;

int check_apply_args(const stl_shamap_tree* t, const void* key, const void* leaf, size_t n, const void* root,
                     const void* counts, bool device_form) {
  if (!t || !root || n > STL_SHAMAP_MAX_ITEMS || (n && !key)) return STL_EINVAL;
  if (!device_form) return STL_OK;  // host arrays: any alignment serves
  if (((uintptr_t)key & 15u) != 0 || ((uintptr_t)leaf & 15u) != 0) return STL_EINVAL;
  if (((uintptr_t)root & 3u) != 0 || ((uintptr_t)counts & 3u) != 0) return STL_EINVAL;
  return STL_OK;
}

int check_fork_args(const stl_shamap_tree* src, const stl_shamap_tree* dst, const void* key, const void* leaf,
                    size_t n, const void* root, const void* counts, bool device_form) {
  if (!src || src == dst) return STL_EINVAL;
  return check_apply_args(dst, key, leaf, n, root, counts, device_form);
}

// One batch of n >= 1 rows on stream s (g_trees.mu held, both trees live on d):
// src's live generation read, dst's other generation written, the work areas
// dst's and the stream context's.  src == dst is an apply, else a fork.
// Enqueued, and waited for only when the host's bound of src's count no longer
// admits the batch into dst.  Nothing of *dst changes here -- the caller
// commits -- and of *src only an apply's own bound.
int tree_enqueue(Device& d, stl_shamap_tree* src, stl_shamap_tree* dst, const uint8_t* d_key, const uint8_t* d_leaf,
                 const uint8_t* d_op, size_t n, uint8_t* d_root, uint32_t* d_counts, hipStream_t s, uint32_t* bound,
                 const ShamapEmit* emit = nullptr) {
  const bool fits = (uint64_t)src->bound + n <= dst->capacity;
  size_t temp = 0, temp_buckets = 0;
  STL_TRY(stl::shamap_temp_bytes(n, &temp));
  STL_TRY(stl::shamap_temp_bytes(stl::kTreeBuckets, &temp_buckets));
  if (temp_buckets > temp) temp = temp_buckets;
  const std::shared_ptr<StreamCtx> c = stream_ctx(d, s);
  std::lock_guard<std::mutex> lk(c->mu);
  STL_RC(c->shamap.ensure(stl::shamap_workspace_bytes(n, temp)));
  STL_RC(dst->batch.ensure(stl::shamap_tree_batch_bytes(n)));
  stl::TreeApply a;
  a.from = src->gen(src->live);
  a.to = dst->gen(dst->live ^ 1);
  a.capacity = dst->capacity;
  a.from_capacity = src->capacity;
  a.items_bound = src->bound;
  a.after_bound = fits ? src->bound + (uint32_t)n : dst->capacity;
  a.fixed = dst->fixed.p;
  a.batch = dst->batch.p;
  a.scratch = dst->scratch.p;
  a.sort_ws = c->shamap.p;
  a.temp_bytes = temp;
  STL_TRY(stl::launch_shamap_tree_locate(a, d_key, d_leaf, d_op, (uint32_t)n, fault_now, phase_clock(d), s));
  if (!fits) {
    // the bound no longer admits the batch: the one wait, for the exact count
    // and what the batch inserts and deletes.  Only the work areas have been
    // written so far, so a refusal leaves the tree as it was.
    uint32_t count = 0, cc[4] = {};
    STL_TRY(hipMemcpyAsync(&count, a.from.meta, 4, hipMemcpyDeviceToHost, s));
    STL_TRY(hipMemcpyAsync(cc, stl::shamap_tree_change_counts(dst->fixed.p), sizeof(cc), hipMemcpyDeviceToHost, s));
    STL_TRY(hipStreamSynchronize(s));
    if (count > src->bound || cc[3] > count || cc[1] > n) return STL_EHIP;
    if (src == dst) src->bound = count;  // a fork only reads its source, the host's bound included
    const uint64_t after = (uint64_t)count - cc[3] + cc[1];
    if (after > dst->capacity) return STL_ENOMEM;
    a.items_bound = count;
    a.after_bound = after ? (uint32_t)after : 1u;
    *bound = (uint32_t)after;
  } else {
    *bound = src->bound + (uint32_t)n;
  }
  STL_TRY(stl::launch_shamap_tree_merge(a, (uint32_t)n, d_root, d_counts, fault_now, phase_clock(d), s, emit));
  return STL_OK;
}

// The fork of no rows (g_trees.mu held, both trees live on d): src's live
// generation copied into dst's other one.  As tree_enqueue: no wait while src's
// bound fits dst, else the one wait for the exact count.
int snapshot_enqueue(const stl_shamap_tree* src, const stl_shamap_tree* dst, uint8_t* d_root, uint32_t* d_counts,
                     uint32_t* d_node_count, hipStream_t s, uint32_t* bound) {
  const stl::TreeGen from = src->gen(src->live);
  uint32_t items = src->bound;
  if (items > dst->capacity) {
    STL_TRY(hipMemcpyAsync(&items, from.meta, 4, hipMemcpyDeviceToHost, s));
    STL_TRY(hipStreamSynchronize(s));
    if (items > src->bound) return STL_EHIP;
    if (items > dst->capacity) return STL_ENOMEM;
  }
  *bound = items;
  STL_TRY(stl::launch_shamap_tree_snapshot(from, src->capacity, items, dst->gen(dst->live ^ 1), dst->capacity, d_root,
                                           d_counts, d_node_count, fault_now, s));
  return STL_OK;
}

// The turn to the generation just written; what a revert needs is kept.
void tree_commit(stl_shamap_tree* t, uint32_t bound_after) {
  t->prev_bound = t->bound;
  t->live ^= 1;
  t->bound = bound_after;
  t->revertible = true;
}

// A call into t failed past its argument checks: the other generation -- the
// one a revert would turn back to -- may be half written.  The tree itself is as
// it was; a revert is refused until the next successful apply or fork into t.
void tree_failed(stl_shamap_tree* t) { t->revertible = false; }

// Both handles live and on the calling thread's device (g_trees.mu held).
int trees_for_call(const stl_shamap_tree* a, const stl_shamap_tree* b, Device** d);

// What the apply and fork entry points share.  src == dst: an apply of the
// batch to the tree; else a fork of src into dst.  out: the nodes form's
// arrays, or null.  A fork of no rows is the snapshot; an apply of no rows
// reports and changes nothing.
int batch_device(stl_shamap_tree* src, stl_shamap_tree* dst, const uint8_t* d_key, const uint8_t* d_leaf,
                 const uint8_t* d_op, size_t n, uint8_t* d_root, uint32_t* d_counts, const stl_shamap_nodes_out* out,
                 void* stream) {
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* d = nullptr;
  STL_RC(trees_for_call(src, dst, &d));
  if (n > dst->capacity) return STL_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* const d_node_count = out ? out->count : nullptr;
  if (n == 0 && src == dst) {
    STL_TRY(stl::launch_shamap_tree_report(dst->gen(dst->live), d_root, d_counts, s, d_node_count));
    return STL_OK;
  }
  uint32_t bound = 0;
  int rc;
  if (n == 0) {
    rc = snapshot_enqueue(src, dst, d_root, d_counts, d_node_count, s, &bound);
  } else if (out) {
    const ShamapEmit emit = emit_of(*out);
    rc = tree_enqueue(*d, src, dst, d_key, d_leaf, d_op, n, d_root, d_counts, s, &bound, &emit);
  } else {
    rc = tree_enqueue(*d, src, dst, d_key, d_leaf, d_op, n, d_root, d_counts, s, &bound);
  }
  if (rc) {
    tree_failed(dst);
    return rc;
  }
  tree_commit(dst, bound);
  return STL_OK;
}

int batch_host(const char* name, stl_shamap_tree* src, stl_shamap_tree* dst, const uint8_t* key, const uint8_t* leaf,
               const uint8_t* op, size_t n, uint8_t root[32], uint32_t counts[8], const stl_shamap_nodes_out* out) {
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* dp = nullptr;
  STL_RC(trees_for_call(src, dst, &dp));
  if (n > dst->capacity) return STL_EINVAL;
  const bool report = n == 0 && src == dst;
  uint32_t bound = 0;
  HostCall call(name, n, *dp);
  const int rc = call.run([&]() -> int {
    Device& d = call.d;
    STL_RC(d.txid.ensure(32));
    STL_RC(d.status.ensure(32));
    NodeStage stage;
    if (out) STL_RC(stage.ensure(d, *out));
    uint8_t* d_root = static_cast<uint8_t*>(d.txid.p);
    uint32_t* d_counts = static_cast<uint32_t*>(d.status.p);
    uint32_t* const d_node_count = out ? stage.emit.count : nullptr;
    if (report) {
      STL_TRY(stl::launch_shamap_tree_report(dst->gen(dst->live), d_root, d_counts, d.stream, d_node_count));
    } else if (n == 0) {
      STL_RC(snapshot_enqueue(src, dst, d_root, d_counts, d_node_count, d.stream, &bound));
    } else {
      STL_RC(call.upload(d.pk, key, n * 32));
      if (leaf) STL_RC(call.upload(d.msg, leaf, n * 32));
      if (op) STL_RC(call.upload(d.sig, op, n));
      STL_RC(tree_enqueue(d, src, dst, static_cast<const uint8_t*>(d.pk.p),
                          leaf ? static_cast<const uint8_t*>(d.msg.p) : nullptr,
                          op ? static_cast<const uint8_t*>(d.sig.p) : nullptr, n, d_root, d_counts, d.stream, &bound,
                          out ? &stage.emit : nullptr));
    }
    call.download(root, d.txid, 32);
    call.download(counts, d.status, 32);
    return out ? stage.fetch(call, *out) : STL_OK;
  });
  if (report) return rc;
  if (rc == STL_OK) tree_commit(dst, bound);  // only once the results are back
  else tree_failed(dst);
  return rc;
}

// ---- the read-only calls: nothing below changes *t ----
int check_lookup_args(const stl_shamap_tree* t, const void* key, size_t n, const void* found, const void* leaf,
                      const void* position, bool device_form) {
  if (!t || n > STL_SHAMAP_MAX_NODES || (n && (!key || !found))) return STL_EINVAL;
  if (!device_form) return STL_OK;  // host arrays: any alignment serves
  if (((uintptr_t)key & 15u) != 0 || ((uintptr_t)leaf & 15u) != 0) return STL_EINVAL;
  if (((uintptr_t)found & 7u) != 0 || ((uintptr_t)position & 3u) != 0) return STL_EINVAL;
  return STL_OK;
}

// The lookup of n >= 1 keys in t's live generation on stream s (g_trees.mu held,
// t live on d): enqueued, never waited for.
int lookup_enqueue(Device& d, const stl_shamap_tree* t, const uint8_t* d_key, size_t n, uint64_t* d_words,
                   uint8_t* d_leaf, uint32_t* d_position, hipStream_t s) {
  size_t temp = 0;
  STL_TRY(stl::shamap_temp_bytes(stl::kTreeBuckets, &temp));
  const std::shared_ptr<StreamCtx> c = stream_ctx(d, s);
  std::lock_guard<std::mutex> lk(c->mu);
  STL_RC(c->shamap.ensure(stl::shamap_lookup_workspace_bytes(temp)));
  STL_TRY(stl::launch_shamap_tree_lookup(t->gen(t->live), t->capacity, d_key, (uint32_t)n, d_words, d_leaf, d_position,
                                         tune_lookup_buckets().load() != 0, c->shamap.p, temp, fault_now, s));
  return STL_OK;
}

int check_compare_args(const stl_shamap_tree* a, const stl_shamap_tree* b, const stl_shamap_diff_out* out,
                       bool device_form) {
  if (!a || !b || !out || out->struct_size != sizeof(stl_shamap_diff_out) || !out->counts) return STL_EINVAL;
  if (out->max_rows > STL_SHAMAP_MAX_NODES || (out->max_rows && (!out->key || !out->kind))) return STL_EINVAL;
  if (!device_form) return STL_OK;
  if ((((uintptr_t)out->key | (uintptr_t)out->leaf_a | (uintptr_t)out->leaf_b) & 15u) != 0) return STL_EINVAL;
  if (((uintptr_t)out->counts & 3u) != 0) return STL_EINVAL;
  return STL_OK;
}

int trees_for_call(const stl_shamap_tree* a, const stl_shamap_tree* b, Device** d) {
  if (!g_trees.live(a) || !g_trees.live(b)) return STL_EINVAL;
  STL_RC(g_trees.for_call(a, d));
  return b->ordinal == a->ordinal ? STL_OK : STL_EINVAL;
}

// The slots a compare is sized for: no more items can differ than both trees hold.
uint32_t compare_slots(const stl_shamap_tree* a, const stl_shamap_tree* b) { return a->bound + b->bound; }

int compare_enqueue(Device& d, const stl_shamap_tree* a, const stl_shamap_tree* b, const stl::ShamapDiff& out,
                    hipStream_t s) {
  const uint32_t slots = compare_slots(a, b);
  size_t temp = 0;
  STL_TRY(stl::shamap_temp_bytes(slots > stl::kTreeBuckets ? slots : stl::kTreeBuckets, &temp));
  const std::shared_ptr<StreamCtx> c = stream_ctx(d, s);
  std::lock_guard<std::mutex> lk(c->mu);
  STL_RC(c->shamap.ensure(stl::shamap_compare_workspace_bytes(slots, temp)));
  STL_TRY(stl::launch_shamap_tree_compare(a->gen(a->live), a->capacity, b->gen(b->live), b->capacity, slots, out,
                                          c->shamap.p, temp, fault_now, s));
  return STL_OK;
}

// ---- the fetch pack: read-only as the two above ----
int check_fetch_args(const stl_shamap_tree* want, const stl_shamap_nodes_out* out, const void* d_counts,
                     bool device_form) {
  STL_RC(check_nodes_out(out, device_form));
  if (!want) return STL_EINVAL;
  if (device_form && ((uintptr_t)d_counts & 3u) != 0) return STL_EINVAL;
  return STL_OK;
}

// want's pack against have (or none) on stream s (g_trees.mu held, the trees
// live on d): enqueued, never waited for; the workspace is the stream context's.
int fetch_enqueue(Device& d, const stl_shamap_tree* want, const stl_shamap_tree* have, const ShamapEmit& emit,
                  uint32_t* d_counts, hipStream_t s) {
  size_t temp = 0;
  STL_TRY(stl::shamap_temp_bytes(stl::kTreeBuckets, &temp));
  const std::shared_ptr<StreamCtx> c = stream_ctx(d, s);
  std::lock_guard<std::mutex> lk(c->mu);
  STL_RC(c->shamap.ensure(stl::shamap_fetch_workspace_bytes(want->bound, have ? have->bound : 0, temp)));
  stl::TreeGen hg{};
  if (have) hg = have->gen(have->live);
  STL_TRY(stl::launch_shamap_tree_fetch_pack(want->gen(want->live), want->capacity, want->bound, have ? &hg : nullptr,
                                             have ? have->capacity : 0, have ? have->bound : 0, emit, d_counts,
                                             c->shamap.p, temp, fault_now, phase_clock(d), s));
  return STL_OK;
}

// ---- nodes by node ID, paths by key: read-only as the three above ----
int check_get_args(const stl_shamap_tree* t, const uint8_t* id, const uint8_t* depth, size_t n, const uint8_t* status,
                   const uint32_t* first, const uint32_t* rows, const uint8_t* leaf_key, const uint8_t* leaf_hash,
                   const stl_shamap_nodes_out* out, const void* counts, bool device_form) {
  STL_RC(check_nodes_out(out, device_form));
  if (!t || n > STL_SHAMAP_GET_MAX_REQUESTS) return STL_EINVAL;
  if (n && (!id || !depth || !status || !first || !rows)) return STL_EINVAL;
  if (!device_form) return STL_OK;  // host arrays: any alignment serves
  if ((((uintptr_t)id | (uintptr_t)leaf_key | (uintptr_t)leaf_hash) & 15u) != 0) return STL_EINVAL;
  if ((((uintptr_t)first | (uintptr_t)rows | (uintptr_t)counts) & 3u) != 0) return STL_EINVAL;
  return STL_OK;
}

// No request: a count of zero and zero counts, nothing else.
int get_nothing(uint32_t* d_count, uint32_t* d_counts, hipStream_t s) {
  STL_TRY(hipMemsetAsync(d_count, 0, 4, s));
  if (d_counts) STL_TRY(hipMemsetAsync(d_counts, 0, 32, s));
  return STL_OK;
}

// n >= 1 requests against t's live generation on stream s (g_trees.mu held, t
// live on d): enqueued, never waited for; the workspace is the stream context's.
int get_enqueue(Device& d, const stl_shamap_tree* t, const stl::ShamapGet& rq, size_t n, const ShamapEmit& emit,
                uint32_t* d_counts, hipStream_t s) {
  size_t temp = 0;
  STL_TRY(stl::shamap_temp_bytes(n > stl::kTreeBuckets ? n : stl::kTreeBuckets, &temp));
  const std::shared_ptr<StreamCtx> c = stream_ctx(d, s);
  std::lock_guard<std::mutex> lk(c->mu);
  STL_RC(c->shamap.ensure(
      stl::shamap_get_workspace_bytes(t->bound, stl::shamap_get_task_rows(n, emit.max_nodes), temp)));
  STL_TRY(stl::launch_shamap_tree_get_nodes(t->gen(t->live), t->capacity, t->bound, rq, (uint32_t)n, emit, d_counts,
                                            c->shamap.p, temp, fault_now, phase_clock(d), s));
  return STL_OK;
}
}  // namespace

extern "C" {

int stl_shamap_tree_create(uint32_t capacity, stl_shamap_tree** out) {
  if (out) *out = nullptr;
  if (!out || capacity == 0 || capacity > STL_SHAMAP_MAX_ITEMS) return STL_EINVAL;
  Device* d = nullptr;
  STL_RC(device_for_call(&d));
  std::unique_ptr<stl_shamap_tree> t(new stl_shamap_tree());
  t->ordinal = d->ordinal;
  t->capacity = capacity;
  DeviceGuard guard;
  auto go = [&]() -> int {
    std::lock_guard<std::mutex> lk(d->mu);
    STL_TRY(hipSetDevice(d->ordinal));
    STL_RC(t->rows[0].ensure(64 * (size_t)capacity));
    STL_RC(t->rows[1].ensure(64 * (size_t)capacity));
    STL_RC(t->genfix.ensure(2 * stl::shamap_tree_gen_fixed_bytes()));
    STL_RC(t->fixed.ensure(stl::shamap_tree_fixed_bytes()));
    STL_RC(t->scratch.ensure(stl::shamap_tree_scratch_bytes(capacity)));
    // the empty tree: no key in any bucket, count zero, root zero -- in both generations
    STL_TRY(hipMemsetAsync(t->genfix.p, 0, 2 * stl::shamap_tree_gen_fixed_bytes(), d->stream));
    STL_TRY(hipStreamSynchronize(d->stream));
    return STL_OK;
  };
  const int rc = go();
  if (rc) {
    (void)hipStreamSynchronize(d->stream);
    t->release();
    return rc;
  }
  g_trees.add(*out = t.release());
  return STL_OK;
}

void stl_shamap_tree_destroy(stl_shamap_tree* t) { g_trees.destroy(t); }

int stl_shamap_tree_get_info(stl_shamap_tree* t, stl_shamap_tree_info* out) {
  if (!out || out->struct_size != sizeof(stl_shamap_tree_info)) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_trees.mu);
  if (!g_trees.live(t)) return STL_EINVAL;
  uint32_t meta[stl::kTreeMetaWords] = {};
  {
    DeviceGuard guard;
    STL_TRY(hipSetDevice(t->ordinal));
    STL_TRY(hipDeviceSynchronize());
    STL_TRY(hipMemcpy(meta, t->gen(t->live).meta, sizeof(meta), hipMemcpyDeviceToHost));
  }
  t->bound = meta[0];
  out->capacity = t->capacity;
  out->items = meta[0];
  out->bucket_depth = stl::kTreeBucketDepth;
  out->device = t->ordinal;
  out->bytes = t->bytes();
  std::memcpy(out->root, meta + stl::kTreeMetaRoot, 32);
  return STL_OK;
}

int stl_shamap_tree_apply_device(stl_shamap_tree* t, const uint8_t* d_key, const uint8_t* d_leaf_hash,
                                 const uint8_t* d_op, size_t n, uint8_t* d_root, uint32_t* d_counts, void* stream) {
  STL_RC(check_apply_args(t, d_key, d_leaf_hash, n, d_root, d_counts, true));
  return batch_device(t, t, d_key, d_leaf_hash, d_op, n, d_root, d_counts, nullptr, stream);
}

int stl_shamap_tree_apply(stl_shamap_tree* t, const uint8_t* key, const uint8_t* leaf_hash, const uint8_t* op,
                          size_t n, uint8_t root[32], uint32_t counts[8]) {
  STL_RC(check_apply_args(t, key, leaf_hash, n, root, counts, false));
  return batch_host("stl_shamap_tree_apply", t, t, key, leaf_hash, op, n, root, counts, nullptr);
}

int stl_shamap_tree_apply_nodes_device(stl_shamap_tree* t, const uint8_t* d_key, const uint8_t* d_leaf_hash,
                                       const uint8_t* d_op, size_t n, uint8_t* d_root, uint32_t* d_counts,
                                       const stl_shamap_nodes_out* out, void* stream) {
  STL_RC(check_apply_args(t, d_key, d_leaf_hash, n, d_root, d_counts, true));
  STL_RC(check_nodes_out(out, true));
  return batch_device(t, t, d_key, d_leaf_hash, d_op, n, d_root, d_counts, out, stream);
}

int stl_shamap_tree_apply_nodes(stl_shamap_tree* t, const uint8_t* key, const uint8_t* leaf_hash, const uint8_t* op,
                                size_t n, uint8_t root[32], uint32_t counts[8], const stl_shamap_nodes_out* out) {
  STL_RC(check_apply_args(t, key, leaf_hash, n, root, counts, false));
  STL_RC(check_nodes_out(out, false));
  return batch_host("stl_shamap_tree_apply_nodes", t, t, key, leaf_hash, op, n, root, counts, out);
}

int stl_shamap_tree_fork_device(stl_shamap_tree* src, stl_shamap_tree* dst, const uint8_t* d_key,
                                const uint8_t* d_leaf_hash, const uint8_t* d_op, size_t n, uint8_t* d_root,
                                uint32_t* d_counts, void* stream) {
  STL_RC(check_fork_args(src, dst, d_key, d_leaf_hash, n, d_root, d_counts, true));
  return batch_device(src, dst, d_key, d_leaf_hash, d_op, n, d_root, d_counts, nullptr, stream);
}

int stl_shamap_tree_fork(stl_shamap_tree* src, stl_shamap_tree* dst, const uint8_t* key, const uint8_t* leaf_hash,
                         const uint8_t* op, size_t n, uint8_t root[32], uint32_t counts[8]) {
  STL_RC(check_fork_args(src, dst, key, leaf_hash, n, root, counts, false));
  return batch_host("stl_shamap_tree_fork", src, dst, key, leaf_hash, op, n, root, counts, nullptr);
}

int stl_shamap_tree_fork_nodes_device(stl_shamap_tree* src, stl_shamap_tree* dst, const uint8_t* d_key,
                                      const uint8_t* d_leaf_hash, const uint8_t* d_op, size_t n, uint8_t* d_root,
                                      uint32_t* d_counts, const stl_shamap_nodes_out* out, void* stream) {
  STL_RC(check_fork_args(src, dst, d_key, d_leaf_hash, n, d_root, d_counts, true));
  STL_RC(check_nodes_out(out, true));
  return batch_device(src, dst, d_key, d_leaf_hash, d_op, n, d_root, d_counts, out, stream);
}

int stl_shamap_tree_fork_nodes(stl_shamap_tree* src, stl_shamap_tree* dst, const uint8_t* key,
                               const uint8_t* leaf_hash, const uint8_t* op, size_t n, uint8_t root[32],
                               uint32_t counts[8], const stl_shamap_nodes_out* out) {
  STL_RC(check_fork_args(src, dst, key, leaf_hash, n, root, counts, false));
  STL_RC(check_nodes_out(out, false));
  return batch_host("stl_shamap_tree_fork_nodes", src, dst, key, leaf_hash, op, n, root, counts, out);
}

int stl_shamap_tree_revert(stl_shamap_tree* t) {
  std::lock_guard<std::mutex> lk(g_trees.mu);
  if (!g_trees.live(t)) return STL_EINVAL;
  // one step, and only to a generation that a successful call left whole
  if (!t->revertible) return STL_EINVAL;
  t->live ^= 1;
  t->bound = t->prev_bound;
  t->revertible = false;
  return STL_OK;
}

int stl_shamap_tree_root_device(stl_shamap_tree* t, uint8_t* d_root, void* stream) {
  if (!t || !d_root || ((uintptr_t)d_root & 3u) != 0) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* d = nullptr;
  STL_RC(g_trees.for_call(t, &d));
  STL_TRY(stl::launch_shamap_tree_report(t->gen(t->live), d_root, nullptr, static_cast<hipStream_t>(stream)));
  return STL_OK;
}

int stl_shamap_tree_export_device(stl_shamap_tree* t, uint8_t* d_key, uint8_t* d_leaf_hash, size_t rows,
                                  uint32_t* d_items, void* stream) {
  if (!t || rows > STL_SHAMAP_MAX_ITEMS) return STL_EINVAL;
  if (((uintptr_t)d_key & 15u) != 0 || ((uintptr_t)d_leaf_hash & 15u) != 0 || ((uintptr_t)d_items & 3u) != 0)
    return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* d = nullptr;
  STL_RC(g_trees.for_call(t, &d));
  if (rows < t->bound) return STL_EINVAL;
  STL_TRY(stl::launch_shamap_tree_export(t->gen(t->live), t->bound, d_key, d_leaf_hash, (uint32_t)rows, d_items,
                                         static_cast<hipStream_t>(stream)));
  return STL_OK;
}

int stl_shamap_tree_lookup_device(stl_shamap_tree* t, const uint8_t* d_key, size_t n, uint64_t* d_found_words,
                                  uint8_t* d_leaf_hash, uint32_t* d_position, void* stream) {
  STL_RC(check_lookup_args(t, d_key, n, d_found_words, d_leaf_hash, d_position, true));
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* d = nullptr;
  STL_RC(g_trees.for_call(t, &d));
  if (n == 0) return STL_OK;
  return lookup_enqueue(*d, t, d_key, n, d_found_words, d_leaf_hash, d_position, static_cast<hipStream_t>(stream));
}

int stl_shamap_tree_lookup(stl_shamap_tree* t, const uint8_t* key, size_t n, uint8_t* found_bitmap,
                           uint8_t* leaf_hash, uint32_t* position) {
  STL_RC(check_lookup_args(t, key, n, found_bitmap, leaf_hash, position, false));
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* dp = nullptr;
  STL_RC(g_trees.for_call(t, &dp));
  if (n == 0) return STL_OK;
  HostCall call("stl_shamap_tree_lookup", n, *dp);
  return call.run([&]() -> int {
    Device& d = call.d;
    STL_RC(call.upload(d.pk, key, n * 32));
    STL_RC(d.bitmap.ensure((n + 63) / 64 * 8));
    if (leaf_hash) STL_RC(d.msg.ensure(n * 32));
    if (position) STL_RC(d.off.ensure(n * 4));
    STL_RC(lookup_enqueue(d, t, static_cast<const uint8_t*>(d.pk.p), n, static_cast<uint64_t*>(d.bitmap.p),
                          leaf_hash ? static_cast<uint8_t*>(d.msg.p) : nullptr,
                          position ? static_cast<uint32_t*>(d.off.p) : nullptr, d.stream));
    call.download(found_bitmap, d.bitmap, (n + 7) / 8);
    call.download(leaf_hash, d.msg, n * 32);
    call.download(position, d.off, n * 4);
    return STL_OK;
  });
}

int stl_shamap_tree_compare_device(stl_shamap_tree* a, stl_shamap_tree* b, const stl_shamap_diff_out* out,
                                   void* stream) {
  STL_RC(check_compare_args(a, b, out, true));
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* d = nullptr;
  STL_RC(trees_for_call(a, b, &d));
  const stl::ShamapDiff diff{out->key, out->kind, out->leaf_a, out->leaf_b, out->max_rows, out->counts};
  return compare_enqueue(*d, a, b, diff, static_cast<hipStream_t>(stream));
}

int stl_shamap_tree_compare(stl_shamap_tree* a, stl_shamap_tree* b, const stl_shamap_diff_out* out) {
  STL_RC(check_compare_args(a, b, out, false));
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* dp = nullptr;
  STL_RC(trees_for_call(a, b, &dp));
  HostCall call("stl_shamap_tree_compare", out->max_rows, *dp);
  return call.run([&]() -> int {
    Device& d = call.d;
    // no more rows can come back than both trees hold
    const uint32_t slots = compare_slots(a, b);
    const uint32_t room = out->max_rows < slots ? out->max_rows : slots;
    const size_t stage = room ? room : 1;  // a place to point at even for no row
    STL_RC(d.pk.ensure(32 * stage));
    STL_RC(d.sig.ensure(stage));
    if (out->leaf_a) STL_RC(d.msg.ensure(32 * stage));
    if (out->leaf_b) STL_RC(d.wide.ensure(32 * stage));
    STL_RC(d.status.ensure(32));
    const stl::ShamapDiff diff{static_cast<uint8_t*>(d.pk.p), static_cast<uint8_t*>(d.sig.p),
                               out->leaf_a ? static_cast<uint8_t*>(d.msg.p) : nullptr,
                               out->leaf_b ? static_cast<uint8_t*>(d.wide.p) : nullptr, room,
                               static_cast<uint32_t*>(d.status.p)};
    STL_RC(compare_enqueue(d, a, b, diff, d.stream));
    uint32_t differences = 0;
    STL_TRY(hipMemcpyAsync(&differences, d.status.p, 4, hipMemcpyDeviceToHost, d.stream));
    STL_TRY(hipStreamSynchronize(d.stream));  // the one wait of its own: how many rows to bring back
    const size_t rows = differences < room ? differences : room;
    call.download(out->counts, d.status, 32);
    if (!rows) return STL_OK;
    call.download(out->key, d.pk, 32 * rows);
    call.download(out->kind, d.sig, rows);
    call.download(out->leaf_a, d.msg, 32 * rows);
    call.download(out->leaf_b, d.wide, 32 * rows);
    return STL_OK;
  });
}

int stl_shamap_tree_fetch_pack_device(stl_shamap_tree* want, stl_shamap_tree* have, const stl_shamap_nodes_out* out,
                                      uint32_t* d_counts, void* stream) {
  STL_RC(check_fetch_args(want, out, d_counts, true));
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* d = nullptr;
  STL_RC(trees_for_call(want, have ? have : want, &d));
  return fetch_enqueue(*d, want, have, emit_of(*out), d_counts, static_cast<hipStream_t>(stream));
}

int stl_shamap_tree_fetch_pack(stl_shamap_tree* want, stl_shamap_tree* have, const stl_shamap_nodes_out* out,
                               uint32_t counts[8]) {
  STL_RC(check_fetch_args(want, out, counts, false));
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* dp = nullptr;
  STL_RC(trees_for_call(want, have ? have : want, &dp));
  HostCall call("stl_shamap_tree_fetch_pack", out->max_nodes, *dp);
  return call.run([&]() -> int {
    Device& d = call.d;
    STL_RC(d.status.ensure(32));
    NodeStage stage;
    STL_RC(stage.ensure(d, *out));
    STL_RC(fetch_enqueue(d, want, have, stage.emit, static_cast<uint32_t*>(d.status.p), d.stream));
    call.download(counts, d.status, 32);
    return stage.fetch(call, *out);
  });
}

int stl_shamap_tree_get_nodes_device(stl_shamap_tree* t, const uint8_t* d_id, const uint8_t* d_depth,
                                     const uint8_t* d_mode, size_t n, uint8_t* d_status, uint32_t* d_first,
                                     uint32_t* d_rows, uint8_t* d_leaf_key, uint8_t* d_leaf_hash,
                                     const stl_shamap_nodes_out* out, uint32_t* d_counts, void* stream) {
  STL_RC(check_get_args(t, d_id, d_depth, n, d_status, d_first, d_rows, d_leaf_key, d_leaf_hash, out, d_counts, true));
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* d = nullptr;
  STL_RC(g_trees.for_call(t, &d));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) return get_nothing(out->count, d_counts, s);
  const stl::ShamapGet rq{d_id, d_depth, d_mode, d_status, d_first, d_rows, d_leaf_key, d_leaf_hash};
  return get_enqueue(*d, t, rq, n, emit_of(*out), d_counts, s);
}

int stl_shamap_tree_get_nodes(stl_shamap_tree* t, const uint8_t* id, const uint8_t* depth, const uint8_t* mode,
                              size_t n, uint8_t* status, uint32_t* first, uint32_t* rows, uint8_t* leaf_key,
                              uint8_t* leaf_hash, const stl_shamap_nodes_out* out, uint32_t counts[8]) {
  STL_RC(check_get_args(t, id, depth, n, status, first, rows, leaf_key, leaf_hash, out, counts, false));
  std::lock_guard<std::mutex> lk(g_trees.mu);
  Device* dp = nullptr;
  STL_RC(g_trees.for_call(t, &dp));
  HostCall call("stl_shamap_tree_get_nodes", n, *dp);
  return call.run([&]() -> int {
    Device& d = call.d;
    STL_RC(d.status.ensure(32));
    NodeStage stage;
    STL_RC(stage.ensure(d, *out));
    uint32_t* const d_counts = static_cast<uint32_t*>(d.status.p);
    if (n == 0) {
      STL_RC(get_nothing(stage.emit.count, d_counts, d.stream));
    } else {
      // the depth bytes, and behind them the mode bytes
      const size_t mode_at = align256(n);
      STL_RC(d.sig.ensure(mode_at + n));
      STL_RC(call.upload(d.pk, id, n * 32));
      STL_RC(call.upload(d.sig, depth, n));
      uint8_t* const d_mode = static_cast<uint8_t*>(d.sig.p) + mode_at;
      if (mode) STL_TRY(hipMemcpyAsync(d_mode, mode, n, hipMemcpyHostToDevice, d.stream));
      STL_RC(d.bitmap.ensure(n));
      STL_RC(d.txid.ensure(4 * n));
      STL_RC(d.gather.ensure(4 * n));
      if (leaf_key) STL_RC(d.msg.ensure(32 * n));
      if (leaf_hash) STL_RC(d.wide.ensure(32 * n));
      const stl::ShamapGet rq{static_cast<const uint8_t*>(d.pk.p),
                              static_cast<const uint8_t*>(d.sig.p),
                              mode ? d_mode : nullptr,
                              static_cast<uint8_t*>(d.bitmap.p),
                              static_cast<uint32_t*>(d.txid.p),
                              static_cast<uint32_t*>(d.gather.p),
                              leaf_key ? static_cast<uint8_t*>(d.msg.p) : nullptr,
                              leaf_hash ? static_cast<uint8_t*>(d.wide.p) : nullptr};
      STL_RC(get_enqueue(d, t, rq, n, stage.emit, d_counts, d.stream));
      call.download(status, d.bitmap, n);
      call.download(first, d.txid, 4 * n);
      call.download(rows, d.gather, 4 * n);
      call.download(leaf_key, d.msg, 32 * n);
      call.download(leaf_hash, d.wide, 32 * n);
    }
    call.download(counts, d.status, 32);
    return stage.fetch(call, *out);  // the one wait of its own: how many rows to bring back
  });
}

}  // extern "C"
