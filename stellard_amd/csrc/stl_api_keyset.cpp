// stl_api_keyset.cpp -- registered signer sets: the stl_keyset_* entry points
// of include/stl.h (kernels: stl_keyset.hip).
#include <algorithm>

#include "stl_host.h"
#include "stl_keyset.h"
#include "stl_keyset_map.h"

using namespace stl;

// One keyset: the keys (host), their first-index map, and on one device the
// records and tables of its nkeys keys plus the base point's (stl_keyset.h).
struct stl_keyset {
  int ordinal = -1;
  uint32_t nkeys = 0;
  std::vector<uint8_t> pk;
  std::map<std::array<uint8_t, 32>, uint32_t> first;
  DevBuf rec, tables;
  // the key -> first index map for the device (stl_keyset_map.h): built from
  // `first`, with the seed and longest probe sequence the builder settled on
  // (map_bound: the bound it had to keep), and its copy on the device
  stl::KeysetMap map;
  uint32_t map_bound = stl::kKsMapProbeBound;
  DevBuf map_dev;
  stl::KeysetMapDev d_map() const {
    return stl::KeysetMapDev{static_cast<const uint32_t*>(map_dev.p), map.mask(), map.longest, map.seed};
  }
  size_t table_bytes() const { return ((size_t)nkeys + 1) * stl::keyset_key_words() * 4; }
  const uint32_t* d_rec() const { return static_cast<const uint32_t*>(rec.p); }
  const uint32_t* d_tables() const { return static_cast<const uint32_t*>(tables.p); }
  void release() {
    rec.release();
    tables.release();
    map_dev.release();
  }
};

namespace {
// Handle first: a call on a destroyed keyset is STL_EINVAL on any thread
// (tests/test_keyset_host.py).
LiveSet<stl_keyset, CheckFirst::kHandle> g_keysets;

// B's encoding (y = 4/5, x positive): the base point's table is built by the
// keys' kernels from it
void base_point_bytes(uint8_t out[32]) {
  std::memset(out, 0x66, 32);
  out[0] = 0x58;
}

// Decodes the keys and builds the tables of `ks` on d.stream (d.mu held).
// `all` (the keys and B's encoding, the copy's source), dpk and scratch are
// the caller's: they outlive the stream's work also when a call here fails.
int keyset_build(Device& d, stl_keyset& ks, std::vector<uint8_t>& all, DevBuf& dpk, DevBuf& scratch) {
  const uint32_t nk = ks.nkeys;
  STL_TRY(hipSetDevice(d.ordinal));
  STL_RC(ks.rec.ensure(((size_t)nk + 1) * stl::keyset_rec_words() * 4));
  STL_RC(ks.tables.ensure(ks.table_bytes()));
  STL_RC(dpk.ensure(((size_t)nk + 1) * 32));
  // the build runs `step` keys at a time: the normalisation's scratch stays small
  const uint32_t step = std::min<uint32_t>(nk + 1, 512);
  STL_RC(scratch.ensure((size_t)step * stl::keyset_scratch_words_per_key() * 4));
  all = ks.pk;
  all.resize(((size_t)nk + 1) * 32);
  base_point_bytes(&all[(size_t)nk * 32]);
  STL_RC(ks.map_dev.ensure(ks.map.slots.size() * 4));
  STL_TRY(hipMemcpyAsync(dpk.p, all.data(), all.size(), hipMemcpyHostToDevice, d.stream));
  // the map goes up with the records (ks.map.slots is the keyset's own: it outlives the copy)
  STL_TRY(hipMemcpyAsync(ks.map_dev.p, ks.map.slots.data(), ks.map.slots.size() * 4, hipMemcpyHostToDevice, d.stream));
  STL_TRY(hipMemsetAsync(ks.tables.p, 0, ks.table_bytes(), d.stream));
  STL_TRY(stl::launch_keyset_decode(static_cast<const uint8_t*>(dpk.p), nk, static_cast<uint32_t*>(ks.rec.p), d.stream));
  for (uint32_t first = 0; first <= nk; first += step)
    STL_TRY(stl::launch_keyset_build(ks.d_rec(), first, std::min<uint32_t>(step, nk + 1 - first),
                                     static_cast<uint32_t*>(ks.tables.p), static_cast<uint32_t*>(scratch.p),
                                     d.stream));
  STL_TRY(hipStreamSynchronize(d.stream));
  return STL_OK;
}

int keyset_launch(Device& d, const stl_keyset& ks, const uint32_t* d_key_index, const uint8_t* d_sig,
                  const uint8_t* d_msg, size_t n, uint64_t* d_words, uint32_t flags, hipStream_t s) {
  STL_TRY(stl::launch_keyset_verify(d_sig, d_msg, d_key_index, (uint32_t)n, ks.d_rec(), ks.d_tables(), ks.nkeys,
                                    stl::core_policy(stl::kernel_mode(flags)), d_words, dev_counters(d), s));
  return STL_OK;
}

// The by-key verify of n rows on stream s (kl: g_keysets.mu, held; ks live on
// d).  Lookup with the miss list, the count copied to the lease's host-mapped
// word behind an event; the keyset verify of all n rows is enqueued; then the
// one wait -- for that event, with kl released: from here on the keyset is not
// touched again -- and the rows that missed go through verify_misses.
int keyset_by_key(std::unique_lock<std::mutex>& kl, Device& d, const stl_keyset& ks, ByKeyLease& use,
                  const uint8_t* d_pk, const uint8_t* d_sig, const uint8_t* d_msg, size_t n, uint64_t* d_words,
                  uint32_t flags, hipStream_t s, size_t* misses) {
  ByKeyBufs& b = use.b;
  const size_t list = align256(n * 4);
  STL_RC(miss_counters(b, 256 + 2 * list));
  uint8_t* base = static_cast<uint8_t*>(b.idx.p);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(base);
  uint32_t* key_index = reinterpret_cast<uint32_t*>(base + 256);
  uint32_t* miss_rows = reinterpret_cast<uint32_t*>(base + 256 + list);
  STL_TRY(hipMemsetAsync(cnt, 0, 4, s));
  STL_TRY(stl::launch_keyset_lookup(d_pk, (uint32_t)n, ks.d_map(), ks.d_rec(), key_index, miss_rows, cnt, s));
  STL_TRY(hipMemcpyAsync(b.count, cnt, 4, hipMemcpyDeviceToHost, s));
  STL_TRY(hipEventRecord(b.counted, s));
  STL_RC(keyset_launch(d, ks, key_index, d_sig, d_msg, n, d_words, flags, s));
  kl.unlock();
  STL_TRY(hipEventSynchronize(b.counted));
  const size_t m = __atomic_load_n(b.count, __ATOMIC_ACQUIRE);
  if (m > n) return STL_EHIP;
  if (misses) *misses = m;
  if (m == 0) return STL_OK;
  return verify_misses(d, use, miss_rows, m, d_sig, d_msg, d_pk, d_words, flags, s);
}
}  // namespace

extern "C" {

int stl_keyset_create(const uint8_t* pk, size_t nkeys, uint32_t flags, stl_keyset** out) {
  if (out) *out = nullptr;
  if (!pk || !out || nkeys == 0 || nkeys > STL_KEYSET_MAX_KEYS || flags != 0) return STL_EINVAL;
  Device* d = nullptr;
  STL_RC(device_for_call(&d));
  std::unique_ptr<stl_keyset> ks(new stl_keyset());
  ks->ordinal = d->ordinal;
  ks->nkeys = (uint32_t)nkeys;
  ks->pk.assign(pk, pk + nkeys * 32);
  for (size_t i = 0; i < nkeys; ++i) {
    std::array<uint8_t, 32> a;
    std::memcpy(a.data(), pk + 32 * i, 32);
    ks->first.emplace(a, (uint32_t)i);  // keeps the first index of a duplicate
  }
  {
    // the device's map, from `first`: a lookup there answers as stl_keyset_find
    std::vector<uint32_t> firsts;
    firsts.reserve(ks->first.size());
    for (const auto& kv : ks->first) firsts.push_back(kv.second);
    std::sort(firsts.begin(), firsts.end());
    std::vector<uint32_t> words(nkeys * 8);
    std::memcpy(words.data(), pk, nkeys * 32);
    if (!stl::keyset_map_build(ks->map, words.data(), (uint32_t)nkeys, firsts.data(), (uint32_t)firsts.size()))
      return STL_EINVAL;  // no seed keeps the probe bound: not reachable by keys that were not made for it
  }
  DeviceGuard guard;
  int rc;
  {
    std::lock_guard<std::mutex> lk(d->mu);
    DevBuf dpk, scratch;
    std::vector<uint8_t> all;
    rc = keyset_build(*d, *ks, all, dpk, scratch);
    if (rc) (void)hipStreamSynchronize(d->stream);  // nothing may still run on the buffers freed below
    dpk.release();
    scratch.release();
    if (rc) ks->release();
  }
  if (rc) return rc;
  g_keysets.add(*out = ks.release());
  return STL_OK;
}

void stl_keyset_destroy(stl_keyset* ks) { g_keysets.destroy(ks); }

int stl_keyset_get_info(const stl_keyset* ks, stl_keyset_info* out) {
  if (!out || out->struct_size != sizeof(stl_keyset_info)) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_keysets.mu);
  if (!g_keysets.live(ks)) return STL_EINVAL;
  const stl::KeysetGeometry g = stl::keyset_geometry();
  out->nkeys = ks->nkeys;
  out->window_bits = g.window_bits;
  out->windows = g.windows;
  out->rows_per_window = g.rows_per_window;
  out->row_bytes = g.row_bytes;
  out->device = ks->ordinal;
  out->reserved = 0;
  out->table_bytes = ks->table_bytes();
  return STL_OK;
}

long long stl_keyset_find(const stl_keyset* ks, const uint8_t pk[32]) {
  std::lock_guard<std::mutex> lk(g_keysets.mu);
  if (!pk || !g_keysets.live(ks)) return -1;
  std::array<uint8_t, 32> a;
  std::memcpy(a.data(), pk, 32);
  const auto it = ks->first.find(a);
  return it == ks->first.end() ? -1 : (long long)it->second;
}

int stl_keyset_verify_batch_device(stl_keyset* ks, const uint32_t* d_key_index, const uint8_t* d_sig,
                                   const uint8_t* d_msg, size_t n, uint64_t* d_bitmap_words, uint32_t flags,
                                   void* stream) {
  if (!ks) return STL_EINVAL;
  STL_RC(check_keyset_flags(flags));
  if (n > 0xffffffc0ull || (n && (!d_key_index || !d_sig || !d_msg || !d_bitmap_words))) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_keysets.mu);
  Device* d = nullptr;
  STL_RC(g_keysets.for_call(ks, &d));
  if (n == 0) return STL_OK;
  return keyset_launch(*d, *ks, d_key_index, d_sig, d_msg, n, d_bitmap_words, flags, static_cast<hipStream_t>(stream));
}

int stl_keyset_tx_verify_batch_device(stl_keyset* ks, const uint32_t* d_key_index, const uint8_t* d_preimages,
                                      const uint64_t* d_offset, const uint32_t* d_len, const uint8_t* d_sig, size_t n,
                                      uint64_t* d_bitmap_words, uint32_t flags, void* stream) {
  if (!ks) return STL_EINVAL;
  STL_RC(check_keyset_flags(flags));
  if (n > 0xffffffc0ull ||
      (n && (!d_key_index || !d_preimages || !d_offset || !d_len || !d_sig || !d_bitmap_words)))
    return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_keysets.mu);
  Device* d = nullptr;
  STL_RC(g_keysets.for_call(ks, &d));
  if (n == 0) return STL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const std::shared_ptr<StreamCtx> c = stream_ctx(*d, s);
  std::lock_guard<std::mutex> cl(c->mu);
  uint32_t* ctr = nullptr;
  STL_RC(ctx_queue(*c, n, &ctr));
  STL_RC(c->scratch.ensure(n * 32));  // the signing hashes
  uint8_t* msg = static_cast<uint8_t*>(c->scratch.p);
  STL_TRY(stl::launch_tx_hash(d_preimages, d_offset, d_len, (uint32_t)n, msg, ctr, hash_grid(*d), s,
                              hash_long_min(*d, n)));
  return keyset_launch(*d, *ks, d_key_index, d_sig, msg, n, d_bitmap_words, flags, s);
}

int stl_keyset_verify_batch(stl_keyset* ks, const uint32_t* key_index, const uint8_t* sig, const uint8_t* msg,
                            size_t n, uint8_t* accept_bitmap, uint32_t flags) {
  if (!ks) return STL_EINVAL;
  STL_RC(check_keyset_flags(flags));
  if (n > 0xffffffc0ull || (n && (!key_index || !sig || !msg || !accept_bitmap))) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_keysets.mu);
  Device* dp = nullptr;
  STL_RC(g_keysets.for_call(ks, &dp));
  if (n == 0) return STL_OK;
  for (size_t i = 0; i < n; ++i)
    if (key_index[i] >= ks->nkeys) return STL_EINVAL;
  HostCall call("stl_keyset_verify_batch", n, *dp);
  return call.run([&]() -> int {
    Device& d = call.d;
    STL_RC(call.upload(d.sig, sig, n * 64));
    STL_RC(call.upload(d.msg, msg, n * 32));
    STL_RC(call.upload(d.len, key_index, n * 4));
    STL_RC(d.bitmap.ensure((n + 63) / 64 * 8));
    STL_RC(keyset_launch(d, *ks, static_cast<const uint32_t*>(d.len.p), static_cast<const uint8_t*>(d.sig.p),
                         static_cast<const uint8_t*>(d.msg.p), n, static_cast<uint64_t*>(d.bitmap.p), flags, d.stream));
    call.download(accept_bitmap, d.bitmap, (n + 7) / 8);
    return STL_OK;
  });
}

int stl_keyset_lookup_device(stl_keyset* ks, const uint8_t* d_pk, size_t n, uint32_t* d_key_index,
                             uint32_t* d_miss_count, void* stream) {
  if (!ks) return STL_EINVAL;
  if (n > 0xffffffc0ull || (n && (!d_pk || !d_key_index))) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_keysets.mu);
  Device* d = nullptr;
  STL_RC(g_keysets.for_call(ks, &d));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d_miss_count) STL_TRY(hipMemsetAsync(d_miss_count, 0, 4, s));
  if (n == 0) return STL_OK;
  STL_TRY(stl::launch_keyset_lookup(d_pk, (uint32_t)n, ks->d_map(), ks->d_rec(), d_key_index, nullptr, d_miss_count,
                                    s));
  return STL_OK;
}

int stl_keyset_verify_by_key_device(stl_keyset* ks, const uint8_t* d_pk, const uint8_t* d_sig, const uint8_t* d_msg,
                                    size_t n, uint64_t* d_bitmap_words, uint32_t flags, void* stream,
                                    size_t* misses) {
  if (misses) *misses = 0;
  if (!ks) return STL_EINVAL;
  STL_RC(check_keyset_flags(flags));
  if (n > 0xffffffc0ull || (n && (!d_pk || !d_sig || !d_msg || !d_bitmap_words))) return STL_EINVAL;
  std::unique_lock<std::mutex> kl(g_keysets.mu);
  Device* d = nullptr;
  STL_RC(g_keysets.for_call(ks, &d));
  if (n == 0) return STL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ByKeyLease use(stream_ctx(*d, s), s);
  return keyset_by_key(kl, *d, *ks, use, d_pk, d_sig, d_msg, n, d_bitmap_words, flags, s, misses);
}

int stl_keyset_signed_blob_verify_batch_device(stl_keyset* ks, uint32_t kind, const uint8_t* d_blobs,
                                               const uint64_t* d_offset, const uint32_t* d_len, size_t n,
                                               uint64_t* d_bitmap_words, uint8_t* d_status, uint8_t* d_id,
                                               uint32_t flags, void* stream, size_t* misses) {
  if (misses) *misses = 0;
  if (!ks) return STL_EINVAL;
  if (kind != STL_BLOB_TRANSACTION && kind != STL_BLOB_VALIDATION) return STL_EINVAL;
  STL_RC(check_keyset_flags(flags));
  if (n > 0xffffffc0ull || (n && (!d_blobs || !d_offset || !d_len || !d_bitmap_words || !d_status)))
    return STL_EINVAL;
  std::unique_lock<std::mutex> kl(g_keysets.mu);
  Device* d = nullptr;
  STL_RC(g_keysets.for_call(ks, &d));
  if (n == 0) return STL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ByKeyLease use(stream_ctx(*d, s), s);
  STL_RC(use.b.blob.ensure(n * 128));  // signing hashes, then signatures, then keys
  uint8_t* msg = static_cast<uint8_t*>(use.b.blob.p);
  uint8_t* sig = msg + 32 * n;
  uint8_t* pk = msg + 96 * n;
  STL_RC(blob_prepare(*d, *use.c, kind, d_blobs, d_offset, d_len, n, msg, sig, pk, d_id, d_status, s));
  return keyset_by_key(kl, *d, *ks, use, pk, sig, msg, n, d_bitmap_words, flags, s, misses);
}

int stl_keyset_verify_by_key(stl_keyset* ks, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, size_t n,
                             uint8_t* accept_bitmap, uint32_t flags) {
  if (!ks) return STL_EINVAL;
  STL_RC(check_keyset_flags(flags));
  if (n > 0xffffffc0ull || (n && (!pk || !sig || !msg || !accept_bitmap))) return STL_EINVAL;
  std::unique_lock<std::mutex> kl(g_keysets.mu);
  Device* dp = nullptr;
  STL_RC(g_keysets.for_call(ks, &dp));
  if (n == 0) return STL_OK;
  HostCall call("stl_keyset_verify_by_key", n, *dp);
  return call.run([&]() -> int {
    Device& d = call.d;
    STL_RC(call.upload(d.sig, sig, n * 64));
    STL_RC(call.upload(d.msg, msg, n * 32));
    STL_RC(call.upload(d.pk, pk, n * 32));
    STL_RC(d.bitmap.ensure((n + 63) / 64 * 8));
    ByKeyLease use(stream_ctx(d, d.stream), d.stream);  // back in its context before the results are fetched
    STL_RC(keyset_by_key(kl, d, *ks, use, static_cast<const uint8_t*>(d.pk.p), static_cast<const uint8_t*>(d.sig.p),
                         static_cast<const uint8_t*>(d.msg.p), n, static_cast<uint64_t*>(d.bitmap.p), flags, d.stream,
                         nullptr));
    call.download(accept_bitmap, d.bitmap, (n + 7) / 8);
    return STL_OK;
  });
}

int stl_debug_keyset_rows(const stl_keyset* ks, uint32_t key, uint32_t first_row, uint32_t nrows,
                          uint32_t* out_words) {
  if (!out_words) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_keysets.mu);
  Device* d = nullptr;
  STL_RC(g_keysets.for_call(ks, &d));
  const stl::KeysetGeometry g = stl::keyset_geometry();
  const uint64_t rows = (uint64_t)g.windows * g.rows_per_window;
  if (key == STL_KEYSET_BASE) key = ks->nkeys;
  else if (key >= ks->nkeys) return STL_EINVAL;
  if ((uint64_t)first_row + nrows > rows) return STL_EINVAL;
  if (nrows == 0) return STL_OK;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(ks->d_tables()) +
                       ((size_t)key * rows + first_row) * g.row_bytes;
  STL_TRY(hipDeviceSynchronize());
  STL_TRY(hipMemcpy(out_words, src, (size_t)nrows * g.row_bytes, hipMemcpyDeviceToHost));
  return STL_OK;
}

}  // extern "C"
