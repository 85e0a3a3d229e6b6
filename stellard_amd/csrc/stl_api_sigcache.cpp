// stl_api_sigcache.cpp -- the verified-ID cache (rows already accepted skip the
// verify): the stl_sigcache_* entry points of include/stl.h; kernels: stl_sigcache.hip.
#include <random>

#include "stl_host.h"
#include "stl_sigcache.h"
#include "stl_sigcache_core.h"

using namespace stl;

// One cache: on one device the lines (stl_sigcache_core.h), and what it is
// bound to -- the blob kind and the accept predicate of the rows it may hold.
struct stl_sigcache {
  int ordinal = -1;
  uint32_t sets_log2 = 0, kind = 0, predicate = 0;
  uint64_t seed = 0;
  DevBuf lines;
  stl::SigCacheDev dev() const {
    return stl::SigCacheDev{static_cast<uint32_t*>(lines.p), (1u << sets_log2) - 1u, seed};
  }
  void release() { lines.release(); }
};

namespace {
// Device first: without a device STL_ENODEV comes before the handle is looked
// at (tests/test_sigcache_host.py).
LiveSet<stl_sigcache, CheckFirst::kDevice> g_sigcaches;

// The cached blob verify of n rows on stream s (kl: g_sigcaches.mu, held; c
// live on d).  The blob pass into the lease's buffers, the probe with the miss
// list, both counts copied to the lease's host-mapped words behind an event;
// then the one wait -- for that event, with kl released -- and the rows that
// missed go through verify_misses, their bits ORed into the bitmap the probe
// wrote.  The insert comes last, under kl again (the handle looked up anew:
// the lines must still be there; `hold`: the host form, which also holds its
// device's mutex, keeps kl throughout instead, by the lock order), and only
// after every earlier step was enqueued without an error: the compact bitmap
// it reads is then written in full by this call's verify, so a failed call
// leaves inserts out but never adds an ID whose verify did not run.
int sigcache_verify(std::unique_lock<std::mutex>& kl, Device& d, const stl_sigcache* c, ByKeyLease& use,
                    const uint8_t* d_blobs, const uint64_t* d_offset, const uint32_t* d_len, size_t n,
                    uint64_t* d_words, uint8_t* d_status, uint8_t* d_id, uint32_t flags, hipStream_t s,
                    size_t* hits, size_t* verified, bool hold = false) {
  ByKeyBufs& b = use.b;
  const stl::SigCacheDev cd = c->dev();
  // signing hashes, signatures, keys; then the IDs when the caller takes none
  STL_RC(b.blob.ensure(n * (d_id ? 128 : 160)));
  uint8_t* msg = static_cast<uint8_t*>(b.blob.p);
  uint8_t* sig = msg + 32 * n;
  uint8_t* pk = msg + 96 * n;
  uint8_t* ids = d_id ? d_id : msg + 128 * n;
  STL_RC(blob_prepare(d, *use.c, c->kind, d_blobs, d_offset, d_len, n, msg, sig, pk, ids, d_status, s));
  STL_RC(miss_counters(b, 256 + align256(n * 4)));
  uint8_t* base = static_cast<uint8_t*>(b.idx.p);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(base);  // [0] misses, [1] hits
  uint32_t* miss_rows = reinterpret_cast<uint32_t*>(base + 256);
  STL_TRY(hipMemsetAsync(cnt, 0, 8, s));
  STL_TRY(stl::launch_sigcache_probe(cd, ids, d_status, (uint32_t)n, d_words, miss_rows, cnt, dev_counters(d), s));
  STL_TRY(hipMemcpyAsync(b.count, cnt, 8, hipMemcpyDeviceToHost, s));
  STL_TRY(hipEventRecord(b.counted, s));
  if (!hold) kl.unlock();
  // the call's one host wait: the per-signature kernels are sized by the miss count
  STL_TRY(hipEventSynchronize(b.counted));
  const size_t m = __atomic_load_n(&b.count[0], __ATOMIC_ACQUIRE);
  const size_t h = __atomic_load_n(&b.count[1], __ATOMIC_ACQUIRE);
  if (m + h > n) return STL_EHIP;
  if (hits) *hits = h;
  if (verified) *verified = m;
  if (m == 0) return STL_OK;  // every decidable row a hit: no per-signature kernel
  const uint64_t* compact = nullptr;
  STL_RC(verify_misses(d, use, miss_rows, m, sig, msg, pk, d_words, flags, s, &compact));
  if (!hold) kl.lock();
  if (!g_sigcaches.live(c)) return STL_OK;  // destroyed during the wait: the outputs stand, nothing to insert into
  STL_TRY(stl::launch_sigcache_insert(cd, miss_rows, (uint32_t)m, compact, ids, s));
  return STL_OK;
}

int check_sigcache_rows(const void* blobs, const void* offset, const void* len, size_t n, const void* bitmap,
                        const void* status, const void* id, uint32_t flags) {
  if (n > 0xffffffc0ull || (n && (!blobs || !offset || !len || !bitmap || !status))) return STL_EINVAL;
  if (((uintptr_t)id & 15u) != 0) return STL_EINVAL;
  return check_flags(flags);
}
}  // namespace

extern "C" {

int stl_sigcache_create(uint32_t sets_log2, uint32_t kind, uint32_t flags, uint64_t seed, stl_sigcache** out) {
  if (out) *out = nullptr;
  if (!out || sets_log2 > STL_SIGCACHE_MAX_SETS_LOG2) return STL_EINVAL;
  if (kind != STL_BLOB_TRANSACTION && kind != STL_BLOB_VALIDATION) return STL_EINVAL;
  STL_RC(check_keyset_flags(flags));  // the predicate bits; no execution flag belongs to a cache
  Device* d = nullptr;
  STL_RC(device_for_call(&d));
  while (seed == 0) {
    std::random_device rd;
    seed = ((uint64_t)rd() << 32) ^ rd();
  }
  std::unique_ptr<stl_sigcache> c(new stl_sigcache());
  c->ordinal = d->ordinal;
  c->sets_log2 = sets_log2;
  c->kind = kind;
  c->predicate = stl::sigcache_predicate(flags);
  c->seed = seed;
  const size_t bytes = stl::sigcache_bytes(sets_log2);
  DeviceGuard guard;
  auto go = [&]() -> int {
    std::lock_guard<std::mutex> lk(d->mu);
    STL_TRY(hipSetDevice(d->ordinal));
    STL_RC(c->lines.ensure(bytes));
    STL_TRY(hipMemsetAsync(c->lines.p, 0, bytes, d->stream));
    STL_TRY(hipStreamSynchronize(d->stream));
    return STL_OK;
  };
  const int rc = go();
  if (rc) {
    (void)hipStreamSynchronize(d->stream);
    c->lines.release();
    return rc;
  }
  g_sigcaches.add(*out = c.release());
  return STL_OK;
}

void stl_sigcache_destroy(stl_sigcache* c) { g_sigcaches.destroy(c); }

int stl_sigcache_get_info(const stl_sigcache* c, stl_sigcache_info* out) {
  if (!out || out->struct_size != sizeof(stl_sigcache_info)) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_sigcaches.mu);
  if (!g_sigcaches.live(c)) return STL_EINVAL;
  out->sets_log2 = c->sets_log2;
  out->ways = STL_SIGCACHE_WAYS;
  out->kind = c->kind;
  out->predicate = c->predicate;
  out->device = c->ordinal;
  out->bytes = stl::sigcache_bytes(c->sets_log2);
  out->seed = c->seed;
  return STL_OK;
}

int stl_sigcache_clear(stl_sigcache* c, void* stream) {
  if (!c) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_sigcaches.mu);
  Device* d = nullptr;
  STL_RC(g_sigcaches.for_call(c, &d));
  STL_TRY(hipMemsetAsync(c->lines.p, 0, stl::sigcache_bytes(c->sets_log2), static_cast<hipStream_t>(stream)));
  return STL_OK;
}

int stl_sigcache_lookup_device(stl_sigcache* c, const uint8_t* d_id, size_t n, uint64_t* d_hit_words, void* stream) {
  if (!c) return STL_EINVAL;
  if (n > 0xffffffc0ull || (n && (!d_id || !d_hit_words)) || ((uintptr_t)d_id & 15u) != 0) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_sigcaches.mu);
  Device* d = nullptr;
  STL_RC(g_sigcaches.for_call(c, &d));
  if (n == 0) return STL_OK;
  STL_TRY(stl::launch_sigcache_lookup(c->dev(), d_id, (uint32_t)n, d_hit_words, static_cast<hipStream_t>(stream)));
  return STL_OK;
}

int stl_sigcache_signed_blob_verify_batch_device(stl_sigcache* c, const uint8_t* d_blobs, const uint64_t* d_offset,
                                                 const uint32_t* d_len, size_t n, uint64_t* d_bitmap_words,
                                                 uint8_t* d_status, uint8_t* d_id, uint32_t flags, void* stream,
                                                 size_t* hits, size_t* verified) {
  if (hits) *hits = 0;
  if (verified) *verified = 0;
  if (!c) return STL_EINVAL;
  STL_RC(check_sigcache_rows(d_blobs, d_offset, d_len, n, d_bitmap_words, d_status, d_id, flags));
  std::unique_lock<std::mutex> kl(g_sigcaches.mu);
  Device* d = nullptr;
  STL_RC(g_sigcaches.for_call(c, &d));
  if (stl::sigcache_predicate(flags) != c->predicate) return STL_EINVAL;
  if (n == 0) return STL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ByKeyLease use(stream_ctx(*d, s), s);
  return sigcache_verify(kl, *d, c, use, d_blobs, d_offset, d_len, n, d_bitmap_words, d_status, d_id, flags, s, hits,
                         verified);
}

int stl_sigcache_signed_blob_verify_batch(stl_sigcache* c, const uint8_t* blobs, const uint64_t* offset,
                                          const uint32_t* len, size_t n, uint8_t* accept_bitmap, uint8_t* status,
                                          uint8_t* id, uint32_t flags, size_t* hits, size_t* verified) {
  if (hits) *hits = 0;
  if (verified) *verified = 0;
  if (!c) return STL_EINVAL;
  STL_RC(check_sigcache_rows(blobs, offset, len, n, accept_bitmap, status, nullptr, flags));
  std::unique_lock<std::mutex> kl(g_sigcaches.mu);
  Device* dp = nullptr;
  STL_RC(g_sigcaches.for_call(c, &dp));
  if (stl::sigcache_predicate(flags) != c->predicate) return STL_EINVAL;
  if (n == 0) return STL_OK;
  HostCall call("stl_sigcache_signed_blob_verify_batch", n, *dp);
  return call.run([&]() -> int {
    Device& d = call.d;
    STL_RC(call.rows(blobs, offset, len, n));
    STL_RC(d.bitmap.ensure((n + 63) / 64 * 8));
    STL_RC(d.status.ensure(n));
    if (id) STL_RC(d.txid.ensure(n * 32));
    if (id) STL_TRY(hipMemsetAsync(d.txid.p, 0, n * 32, d.stream));  // a malformed row's ID is not written
    ByKeyLease use(stream_ctx(d, d.stream), d.stream);  // back in its context before the results are fetched
    STL_RC(sigcache_verify(kl, d, c, use, static_cast<const uint8_t*>(d.pre.p), static_cast<const uint64_t*>(d.off.p),
                           static_cast<const uint32_t*>(d.len.p), n, static_cast<uint64_t*>(d.bitmap.p),
                           static_cast<uint8_t*>(d.status.p), id ? static_cast<uint8_t*>(d.txid.p) : nullptr, flags,
                           d.stream, hits, verified, true));
    call.download(accept_bitmap, d.bitmap, (n + 7) / 8);
    call.download(status, d.status, n);
    call.download(id, d.txid, 32 * n);
    return STL_OK;
  });
}

}  // extern "C"
