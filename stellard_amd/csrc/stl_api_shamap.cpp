// stl_api_shamap.cpp -- the SHAMap root of a set of keys (the hash a node
// compares for a transaction set): the stl_shamap_root* entry points of
// include/stl.h; kernels: stl_shamap.hip.
#include "stl_host.h"
#include "stl_shamap.h"

using namespace stl;

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
                   size_t n, uint8_t* d_root, uint32_t* d_counts, hipStream_t s) {
  size_t temp = 0;
  STL_TRY(stl::shamap_temp_bytes(n, &temp));
  STL_RC(c.shamap.ensure(stl::shamap_workspace_bytes(n, temp)));
  STL_TRY(stl::launch_shamap_root(d_key, d_leaf, d_select, (uint32_t)n, d_root, d_counts, c.shamap.p, temp, fault_now,
                                  phase_clock(d), s));
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

}  // extern "C"
