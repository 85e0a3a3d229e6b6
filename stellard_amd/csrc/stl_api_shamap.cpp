// stl_api_shamap.cpp -- the SHAMap root of a set of keys (the hash a node
// compares for a transaction set), and the same with the set's inner nodes
// stored: the stl_shamap_root* and stl_shamap_nodes* entry points of
// include/stl.h; kernels: stl_shamap.hip.
#include "stl_host.h"
#include "stl_shamap.h"

using namespace stl;

namespace stl {

int check_nodes_out(const stl_shamap_nodes_out* out, bool device_form) {
  if (!out || out->struct_size != sizeof(stl_shamap_nodes_out)) return STL_EINVAL;
  if (!out->hash || !out->body || !out->count || out->max_nodes > STL_SHAMAP_MAX_NODES) return STL_EINVAL;
  if (!device_form) return STL_OK;  // host arrays: any alignment serves
  if ((((uintptr_t)out->hash | (uintptr_t)out->body | (uintptr_t)out->id) & 15u) != 0) return STL_EINVAL;
  if ((((uintptr_t)out->meta | (uintptr_t)out->count) & 3u) != 0) return STL_EINVAL;
  return STL_OK;
}

ShamapEmit emit_of(const stl_shamap_nodes_out& out) {
  return ShamapEmit{out.hash, out.body, out.id, out.meta, out.max_nodes, out.count};
}

int NodeStage::ensure(Device& d, const stl_shamap_nodes_out& out) {
  const size_t rows = out.max_nodes ? out.max_nodes : 1;  // a place to point at even for no row
  STL_RC(d.off.ensure(32 * rows));
  STL_RC(d.pre.ensure(512 * rows));
  if (out.id) STL_RC(d.len.ensure(32 * rows));
  if (out.meta) STL_RC(d.ctr2.ensure(4 * rows));
  STL_RC(d.ctr.ensure(4));
  emit = ShamapEmit{static_cast<uint8_t*>(d.off.p), static_cast<uint8_t*>(d.pre.p),
                    out.id ? static_cast<uint8_t*>(d.len.p) : nullptr,
                    out.meta ? static_cast<uint32_t*>(d.ctr2.p) : nullptr, out.max_nodes,
                    static_cast<uint32_t*>(d.ctr.p)};
  return STL_OK;
}

int NodeStage::fetch(HostCall& call, const stl_shamap_nodes_out& out) {
  Device& d = call.d;
  uint32_t count = 0;
  STL_TRY(hipMemcpyAsync(&count, d.ctr.p, 4, hipMemcpyDeviceToHost, d.stream));
  STL_TRY(hipStreamSynchronize(d.stream));  // the one wait of its own: how many rows to bring back
  const size_t rows = count < out.max_nodes ? count : out.max_nodes;
  call.download(out.count, d.ctr, 4);
  if (!rows) return STL_OK;
  call.download(out.hash, d.off, 32 * rows);
  call.download(out.body, d.pre, 512 * rows);
  call.download(out.id, d.len, 32 * rows);
  call.download(out.meta, d.ctr2, 4 * rows);
  return STL_OK;
}

}  // namespace stl

namespace {

int check_shamap_args(const void* key, const void* leaf, size_t n, const void* root, const void* counts) {
  if (!root || n > STL_SHAMAP_MAX_ITEMS || (n && !key)) return STL_EINVAL;
  if (((uintptr_t)key & 15u) != 0 || ((uintptr_t)leaf & 15u) != 0) return STL_EINVAL;
  if (((uintptr_t)root & 3u) != 0 || ((uintptr_t)counts & 3u) != 0) return STL_EINVAL;
  return STL_OK;
}

// The root of n >= 1 rows on stream s with context c's workspace (c.mu held):
// enqueued, never waited for.
int shamap_enqueue(Device& d, StreamCtx& c, const uint8_t* d_key, const uint8_t* d_leaf, const uint64_t* d_select,
                   size_t n, uint8_t* d_root, uint32_t* d_counts, hipStream_t s, const ShamapEmit* emit = nullptr) {
  size_t temp = 0;
  STL_TRY(stl::shamap_temp_bytes(n, &temp));
  STL_RC(c.shamap.ensure(stl::shamap_workspace_bytes(n, temp)));
  STL_TRY(stl::launch_shamap_root(d_key, d_leaf, d_select, (uint32_t)n, d_root, d_counts, c.shamap.p, temp, fault_now,
                                  phase_clock(d), s, emit));
  return STL_OK;
}

}  // namespace

extern "C" {

int stl_shamap_root_device(const uint8_t* d_key, const uint8_t* d_leaf_hash, const uint64_t* d_select_words, size_t n,
                           uint8_t* d_root, uint32_t* d_counts, void* stream) {
  STL_RC(check_shamap_args(d_key, d_leaf_hash, n, d_root, d_counts));
  Device* d = nullptr;
  STL_RC(device_for_call(&d));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) {  // the empty map
    STL_TRY(hipMemsetAsync(d_root, 0, 32, s));
    if (d_counts) STL_TRY(hipMemsetAsync(d_counts, 0, 16, s));
    return STL_OK;
  }
  const std::shared_ptr<StreamCtx> c = stream_ctx(*d, s);
  std::lock_guard<std::mutex> lk(c->mu);
  return shamap_enqueue(*d, *c, d_key, d_leaf_hash, d_select_words, n, d_root, d_counts, s);
}

int stl_shamap_root(const uint8_t* key, const uint8_t* leaf_hash, const uint8_t* select_bitmap, size_t n,
                    uint8_t root[32], uint32_t counts[4]) {
  // host arrays: any alignment serves, the copies land in the device's own buffers
  if (!root || n > STL_SHAMAP_MAX_ITEMS || (n && !key)) return STL_EINVAL;
  Device* dp = nullptr;
  STL_RC(device_for_call(&dp));
  if (n == 0) {
    std::memset(root, 0, 32);
    if (counts) std::memset(counts, 0, 16);
    return STL_OK;
  }
  HostCall call("stl_shamap_root", n, *dp);
  return call.run([&]() -> int {
    Device& d = call.d;
    STL_RC(call.upload(d.pk, key, n * 32));
    if (leaf_hash) STL_RC(call.upload(d.msg, leaf_hash, n * 32));
    const size_t words = (n + 63) / 64;
    if (select_bitmap) {
      STL_RC(d.bitmap.ensure(words * 8));
      STL_TRY(hipMemsetAsync(static_cast<uint8_t*>(d.bitmap.p) + (words - 1) * 8, 0, 8, d.stream));
      STL_TRY(hipMemcpyAsync(d.bitmap.p, select_bitmap, (n + 7) / 8, hipMemcpyHostToDevice, d.stream));
    }
    STL_RC(d.txid.ensure(32));
    STL_RC(d.status.ensure(16));
    {
      const std::shared_ptr<StreamCtx> c = stream_ctx(d, d.stream);
      std::lock_guard<std::mutex> lk(c->mu);
      STL_RC(shamap_enqueue(d, *c, static_cast<const uint8_t*>(d.pk.p),
                            leaf_hash ? static_cast<const uint8_t*>(d.msg.p) : nullptr,
                            select_bitmap ? static_cast<const uint64_t*>(d.bitmap.p) : nullptr, n,
                            static_cast<uint8_t*>(d.txid.p), static_cast<uint32_t*>(d.status.p), d.stream));
    }
    call.download(root, d.txid, 32);
    call.download(counts, d.status, 16);
    return STL_OK;
  });
}

int stl_shamap_nodes_device(const uint8_t* d_key, const uint8_t* d_leaf_hash, const uint64_t* d_select_words, size_t n,
                            uint8_t* d_root, uint32_t* d_counts, const stl_shamap_nodes_out* out, void* stream) {
  STL_RC(check_shamap_args(d_key, d_leaf_hash, n, d_root, d_counts));
  STL_RC(check_nodes_out(out, true));
  Device* d = nullptr;
  STL_RC(device_for_call(&d));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) {  // the empty map: no node
    STL_TRY(hipMemsetAsync(d_root, 0, 32, s));
    if (d_counts) STL_TRY(hipMemsetAsync(d_counts, 0, 16, s));
    STL_TRY(hipMemsetAsync(out->count, 0, 4, s));
    return STL_OK;
  }
  const ShamapEmit emit = emit_of(*out);
  const std::shared_ptr<StreamCtx> c = stream_ctx(*d, s);
  std::lock_guard<std::mutex> lk(c->mu);
  return shamap_enqueue(*d, *c, d_key, d_leaf_hash, d_select_words, n, d_root, d_counts, s, &emit);
}

int stl_shamap_nodes(const uint8_t* key, const uint8_t* leaf_hash, const uint8_t* select_bitmap, size_t n,
                     uint8_t root[32], uint32_t counts[4], const stl_shamap_nodes_out* out) {
  if (!root || n > STL_SHAMAP_MAX_ITEMS || (n && !key)) return STL_EINVAL;
  STL_RC(check_nodes_out(out, false));
  Device* dp = nullptr;
  STL_RC(device_for_call(&dp));
  if (n == 0) {
    std::memset(root, 0, 32);
    if (counts) std::memset(counts, 0, 16);
    std::memset(out->count, 0, 4);
    return STL_OK;
  }
  HostCall call("stl_shamap_nodes", n, *dp);
  return call.run([&]() -> int {
    Device& d = call.d;
    STL_RC(call.upload(d.pk, key, n * 32));
    if (leaf_hash) STL_RC(call.upload(d.msg, leaf_hash, n * 32));
    const size_t words = (n + 63) / 64;
    if (select_bitmap) {
      STL_RC(d.bitmap.ensure(words * 8));
      STL_TRY(hipMemsetAsync(static_cast<uint8_t*>(d.bitmap.p) + (words - 1) * 8, 0, 8, d.stream));
      STL_TRY(hipMemcpyAsync(d.bitmap.p, select_bitmap, (n + 7) / 8, hipMemcpyHostToDevice, d.stream));
    }
    STL_RC(d.txid.ensure(32));
    STL_RC(d.status.ensure(16));
    NodeStage stage;
    STL_RC(stage.ensure(d, *out));
    {
      const std::shared_ptr<StreamCtx> c = stream_ctx(d, d.stream);
      std::lock_guard<std::mutex> lk(c->mu);
      STL_RC(shamap_enqueue(d, *c, static_cast<const uint8_t*>(d.pk.p),
                            leaf_hash ? static_cast<const uint8_t*>(d.msg.p) : nullptr,
                            select_bitmap ? static_cast<const uint64_t*>(d.bitmap.p) : nullptr, n,
                            static_cast<uint8_t*>(d.txid.p), static_cast<uint32_t*>(d.status.p), d.stream,
                            &stage.emit));
    }
    call.download(root, d.txid, 32);
    call.download(counts, d.status, 16);
    return stage.fetch(call, *out);
  });
}

}  // extern "C"
