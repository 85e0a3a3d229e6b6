// stl_api_authority.cpp -- who may sign: account IDs and the master-key match
// (stl_signer.hip), the account directory with Transactor::checkSig's verdict per row
// (stl_acctdir.hip): the stl_account_id_*, stl_tx_blob_signer_*, stl_acctdir_* entry points.
#include <algorithm>
#include <random>

#include "stl_acctdir.h"
#include "stl_acctdir_core.h"
#include "stl_host.h"
#include "stl_signer.h"

using namespace stl;

// One directory: on one device the slots, the records and two words of
// bookkeeping (stl_acctdir.h AcctDirDev), plus the staging buffer of upsert.
// The record count is the device's word; `records` is the host's copy, read
// back at the end of every upsert (count_stale: that read has yet to succeed).
struct stl_acctdir {
  int ordinal = -1;
  uint32_t capacity = 0, nslots = 0;
  uint64_t seed = 0;
  uint32_t records = 0, longest_probe = 0;
  bool count_stale = false;
  DevBuf slots, recs, meta, stage;
  stl::AcctDirDev dev() const {
    return stl::AcctDirDev{static_cast<uint32_t*>(slots.p), static_cast<uint32_t*>(recs.p),
                           static_cast<uint32_t*>(meta.p), nslots - 1, capacity, seed};
  }
  size_t bytes() const { return (size_t)nslots * 4 + (size_t)capacity * stl::kAdRecWords * 4; }
  void release() {
    slots.release();
    recs.release();
    meta.release();
    stage.release();
  }
};

namespace {
// Device first: without a device STL_ENODEV comes before the handle is looked
// at (tests/test_acctdir_host.py).
LiveSet<stl_acctdir, CheckFirst::kDevice> g_acctdirs;

// The signer pass over host rows, for stl_tx_blob_signer_batch (no directory:
// the master-key match) and stl_acctdir_tx_blob_authority (checkSig's verdict)
// alike: `launch` is given the rows on the device, the three output buffers
// (an output the caller does not take is null) and the stream.
template <typename Launch>
int signer_host_call(const char* name, Device& dev, Launch launch, const uint8_t* blobs, const uint64_t* offset,
                     const uint32_t* len, size_t n, uint8_t* signer_id, uint8_t* account, uint8_t* authority) {
  HostCall call(name, n, dev);
  return call.run([&]() -> int {
    Device& d = call.d;
    const size_t idb = n * STL_ACCOUNT_ID_BYTES;
    STL_RC(call.rows(blobs, offset, len, n));
    STL_RC(d.msg.ensure(idb));
    STL_RC(d.txid.ensure(idb));
    STL_RC(d.status.ensure(n));
    STL_TRY(launch(static_cast<const uint8_t*>(d.pre.p), static_cast<const uint64_t*>(d.off.p),
                   static_cast<const uint32_t*>(d.len.p), (uint32_t)n,
                   signer_id ? static_cast<uint8_t*>(d.msg.p) : nullptr,
                   account ? static_cast<uint8_t*>(d.txid.p) : nullptr, static_cast<uint8_t*>(d.status.p), d.stream));
    call.download(signer_id, d.msg, idb);
    call.download(account, d.txid, idb);
    call.download(authority, d.status, n);
    return STL_OK;
  });
}

// meta[0 .. 2) -> the host's copy.  Not counted by the fault injection: it
// also runs on upsert's failure path.
bool acctdir_read_meta(stl_acctdir& dir) {
  uint32_t m[2] = {0, 0};
  if (hipMemcpy(m, dir.meta.p, sizeof(m), hipMemcpyDeviceToHost) != hipSuccess) {
    dir.count_stale = true;
    return false;
  }
  dir.records = std::min(m[0], dir.capacity);
  dir.longest_probe = m[1];
  dir.count_stale = false;
  return true;
}
}  // namespace

extern "C" {

// ---- signer authority ----
int stl_account_id_batch_device(const uint8_t* d_pk, size_t n, uint8_t* d_account_id, void* stream) {
  if (n == 0) return STL_OK;
  if (!d_pk || !d_account_id || n > 0xffffffc0ull) return STL_EINVAL;
  // the kernel's 16-byte loads and dword stores: refused, never attempted
  if (((uintptr_t)d_pk & 15u) != 0 || ((uintptr_t)d_account_id & 3u) != 0) return STL_EINVAL;
  Device* d = nullptr;
  STL_RC(device_for_call(&d));
  STL_TRY(stl::launch_account_id(d_pk, (uint32_t)n, d_account_id, static_cast<hipStream_t>(stream)));
  return STL_OK;
}

int stl_tx_blob_signer_batch_device(const uint8_t* d_blobs, const uint64_t* d_offset, const uint32_t* d_len, size_t n,
                                    uint8_t* d_signer_id, uint8_t* d_account, uint8_t* d_authority, void* stream) {
  if (n == 0) return STL_OK;
  if (!d_blobs || !d_offset || !d_len || !d_signer_id || !d_authority || n > 0xffffffc0ull) return STL_EINVAL;
  if (((uintptr_t)d_signer_id & 3u) != 0 || ((uintptr_t)d_account & 3u) != 0) return STL_EINVAL;
  Device* d = nullptr;
  STL_RC(device_for_call(&d));
  STL_TRY(stl::launch_tx_signer(d_blobs, d_offset, d_len, (uint32_t)n, d_signer_id, d_account, d_authority,
                                static_cast<hipStream_t>(stream)));
  return STL_OK;
}

int stl_account_id_batch(const uint8_t* pk, size_t n, uint8_t* account_id) {
  if (n == 0) return STL_OK;
  if (!pk || !account_id || n > 0xffffffc0ull) return STL_EINVAL;
  STL_RC(ensure_init());
  if (g_devs.empty()) return STL_ENODEV;
  HostCall call("stl_account_id_batch", n, *g_devs[0]);
  return call.run([&]() -> int {
    Device& d = call.d;
    STL_RC(call.upload(d.pk, pk, n * 32));
    STL_RC(d.msg.ensure(n * STL_ACCOUNT_ID_BYTES));
    STL_TRY(stl::launch_account_id(static_cast<const uint8_t*>(d.pk.p), (uint32_t)n, static_cast<uint8_t*>(d.msg.p),
                                   d.stream));
    call.download(account_id, d.msg, n * STL_ACCOUNT_ID_BYTES);
    return STL_OK;
  });
}

int stl_tx_blob_signer_batch(const uint8_t* blobs, const uint64_t* offset, const uint32_t* len, size_t n,
                             uint8_t* signer_id, uint8_t* account, uint8_t* authority) {
  if (n == 0) return STL_OK;
  if (!blobs || !offset || !len || !signer_id || !authority || n > 0xffffffc0ull) return STL_EINVAL;
  STL_RC(ensure_init());
  if (g_devs.empty()) return STL_ENODEV;
  return signer_host_call("stl_tx_blob_signer_batch", *g_devs[0], stl::launch_tx_signer, blobs, offset, len, n,
                          signer_id, account, authority);
}

// ---- account directory ----

int stl_acctdir_create(uint32_t capacity, uint64_t seed, stl_acctdir** out) {
  if (out) *out = nullptr;
  if (!out || capacity == 0 || capacity > STL_ACCTDIR_MAX_ACCOUNTS) return STL_EINVAL;
  Device* d = nullptr;
  STL_RC(device_for_call(&d));
  while (seed == 0) {
    std::random_device rd;
    seed = ((uint64_t)rd() << 32) ^ rd();
  }
  std::unique_ptr<stl_acctdir> dir(new stl_acctdir());
  dir->ordinal = d->ordinal;
  dir->capacity = capacity;
  dir->nslots = stl::acctdir_slots(capacity);
  dir->seed = seed;
  DeviceGuard guard;
  auto go = [&]() -> int {
    std::lock_guard<std::mutex> lk(d->mu);
    STL_TRY(hipSetDevice(d->ordinal));
    STL_RC(dir->slots.ensure((size_t)dir->nslots * 4));
    STL_RC(dir->recs.ensure((size_t)capacity * stl::kAdRecWords * 4));
    STL_RC(dir->meta.ensure(8));
    STL_TRY(hipMemsetAsync(dir->slots.p, 0xFF, (size_t)dir->nslots * 4, d->stream));
    STL_TRY(hipMemsetAsync(dir->recs.p, 0, (size_t)capacity * stl::kAdRecWords * 4, d->stream));
    STL_TRY(hipMemsetAsync(dir->meta.p, 0, 8, d->stream));
    STL_TRY(hipStreamSynchronize(d->stream));
    return STL_OK;
  };
  const int rc = go();
  if (rc) {
    (void)hipStreamSynchronize(d->stream);
    dir->release();
    return rc;
  }
  g_acctdirs.add(*out = dir.release());
  return STL_OK;
}

void stl_acctdir_destroy(stl_acctdir* dir) { g_acctdirs.destroy(dir); }

int stl_acctdir_get_info(const stl_acctdir* dir, stl_acctdir_info* out) {
  if (!out || out->struct_size != sizeof(stl_acctdir_info)) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_acctdirs.mu);
  if (!g_acctdirs.live(dir)) return STL_EINVAL;
  if (dir->count_stale) {
    DeviceGuard guard;
    if (hipSetDevice(dir->ordinal) != hipSuccess || !acctdir_read_meta(*const_cast<stl_acctdir*>(dir))) return STL_EHIP;
  }
  out->capacity = dir->capacity;
  out->records = dir->records;
  out->slots = dir->nslots;
  out->longest_probe = dir->longest_probe;
  out->device = dir->ordinal;
  out->bytes = dir->bytes();
  out->seed = dir->seed;
  return STL_OK;
}

int stl_acctdir_upsert(stl_acctdir* dir, const uint8_t* account_id, const uint8_t* flags, const uint8_t* regular_key,
                       size_t m) {
  if (m == 0) return STL_OK;
  if (!dir || !account_id || !flags || m > 0xffffffc0ull) return STL_EINVAL;
  std::vector<uint32_t> staged;
  if (!stl::acctdir_stage(account_id, flags, regular_key, m, staged)) return STL_EINVAL;
  const size_t distinct = staged.size() / stl::kAdRecWords;
  std::lock_guard<std::mutex> lk(g_acctdirs.mu);
  Device* d = nullptr;
  STL_RC(g_acctdirs.for_call(dir, &d));
  DeviceGuard guard;
  std::lock_guard<std::mutex> dl(d->mu);
  if (dir->count_stale && !acctdir_read_meta(*dir)) return STL_EHIP;
  if ((size_t)dir->records + distinct > dir->capacity) return STL_ENOMEM;  // before any device work
  const size_t rec_bytes = distinct * stl::kAdRecWords * 4;
  auto go = [&]() -> int {
    STL_TRY(hipSetDevice(d->ordinal));
    STL_RC(dir->stage.ensure(rec_bytes + distinct * 4));
    uint32_t* d_staged = static_cast<uint32_t*>(dir->stage.p);
    uint32_t* d_new = d_staged + distinct * stl::kAdRecWords;
    STL_TRY(hipMemcpyAsync(d_staged, staged.data(), rec_bytes, hipMemcpyHostToDevice, d->stream));
    STL_TRY(stl::launch_acctdir_find(dir->dev(), d_staged, (uint32_t)distinct, d_new, d->stream));
    STL_TRY(stl::launch_acctdir_claim(dir->dev(), d_staged, (uint32_t)distinct, d_new, d->stream));
    STL_TRY(hipStreamSynchronize(d->stream));
    return STL_OK;
  };
  const int rc = go();
  if (rc) (void)hipStreamSynchronize(d->stream);  // nothing may still read `staged`
  const bool read = acctdir_read_meta(*dir);       // the count moved even where the call failed
  return rc ? rc : (read ? STL_OK : STL_EHIP);
}

int stl_acctdir_lookup_device(stl_acctdir* dir, const uint8_t* d_account_id, size_t n, uint8_t* d_flags,
                              uint8_t* d_regular_key, void* stream) {
  if (n == 0) return STL_OK;
  if (!dir || !d_account_id || !d_flags || n > 0xffffffc0ull) return STL_EINVAL;
  if (((uintptr_t)d_account_id & 3u) != 0 || ((uintptr_t)d_regular_key & 3u) != 0) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_acctdirs.mu);
  Device* d = nullptr;
  STL_RC(g_acctdirs.for_call(dir, &d));
  STL_TRY(stl::launch_acctdir_lookup(dir->dev(), d_account_id, (uint32_t)n, d_flags, d_regular_key,
                                     static_cast<hipStream_t>(stream)));
  return STL_OK;
}

int stl_acctdir_tx_blob_authority_device(stl_acctdir* dir, const uint8_t* d_blobs, const uint64_t* d_offset,
                                         const uint32_t* d_len, size_t n, uint8_t* d_signer_id, uint8_t* d_account,
                                         uint8_t* d_authority, void* stream) {
  if (n == 0) return STL_OK;
  if (!dir || !d_blobs || !d_offset || !d_len || !d_authority || n > 0xffffffc0ull) return STL_EINVAL;
  if (((uintptr_t)d_signer_id & 3u) != 0 || ((uintptr_t)d_account & 3u) != 0) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_acctdirs.mu);
  Device* d = nullptr;
  STL_RC(g_acctdirs.for_call(dir, &d));
  STL_TRY(stl::launch_acctdir_authority(dir->dev(), d_blobs, d_offset, d_len, (uint32_t)n, d_signer_id, d_account,
                                        d_authority, static_cast<hipStream_t>(stream)));
  return STL_OK;
}

int stl_acctdir_tx_blob_authority(stl_acctdir* dir, const uint8_t* blobs, const uint64_t* offset, const uint32_t* len,
                                  size_t n, uint8_t* signer_id, uint8_t* account, uint8_t* authority) {
  if (n == 0) return STL_OK;
  if (!dir || !blobs || !offset || !len || !authority || n > 0xffffffc0ull) return STL_EINVAL;
  std::lock_guard<std::mutex> lk(g_acctdirs.mu);
  Device* dp = nullptr;
  STL_RC(g_acctdirs.for_call(dir, &dp));
  const stl::AcctDirDev dd = dir->dev();
  return signer_host_call(
      "stl_acctdir_tx_blob_authority", *dp,
      [&dd](auto... rows_outputs_stream) { return stl::launch_acctdir_authority(dd, rows_outputs_stream...); }, blobs,
      offset, len, n, signer_id, account, authority);
}

}  // extern "C"
