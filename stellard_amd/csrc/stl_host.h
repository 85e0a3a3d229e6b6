// stl_host.h -- what the host files of libstl share (stl_api.cpp and
// stl_api_keyset.cpp, stl_api_authority.cpp, stl_api_sigcache.cpp,
// stl_api_shamap.cpp): the fault
// countdown and the checked-call macros, the device, stream-context and buffer
// types, the registry of live handle objects, the synchronous host call and
// the by-key calls' miss path.  Host only: no .hip file includes it.  Every
// global and every function declared here is defined once, in stl_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <array>
#include <atomic>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <vector>

#include "../../include/stl.h"
#include "stl_kernels.h"

namespace stl {

// ---- fault injection (stl_debug_fault_after) --------------------------------
// A countdown over the HIP / RCCL calls libstl checks; the call at which it
// reaches zero is not executed and reports failure.  One shot.
bool fault_now();

#define STL_TRY(expr)                        \
  do {                                       \
    if (::stl::fault_now()) return STL_EHIP; \
    hipError_t e_ = (expr);                  \
    if (e_ != hipSuccess) return STL_EHIP;   \
  } while (0)

#define STL_RCCL_TRY(expr)                    \
  do {                                        \
    if (::stl::fault_now()) return STL_ERCCL; \
    ncclResult_t r_ = (expr);                 \
    if (r_ != ncclSuccess) return STL_ERCCL;  \
  } while (0)

#define STL_RC(expr)        \
  do {                      \
    int rc_ = (expr);       \
    if (rc_) return rc_;    \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return STL_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (fault_now() || hipMalloc(&p, bytes) != hipSuccess) {
      p = nullptr;
      return STL_ENOMEM;
    }
    cap = bytes;
    return STL_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Phase timing (stl_set_phase_timing): launch_verify marks the phase
// boundaries of each chunk; each mark records a pooled HIP event on the launch
// stream.  stl_get_stats sums the completed chunks' phase durations.  Timing
// calls bypass the fault-injection countdown and never fail a launch: a chunk
// whose events could not be recorded is dropped from the sums.
struct PhaseTimer {
  std::mutex mu;
  std::vector<hipEvent_t> pool;
  std::vector<std::array<hipEvent_t, 5>> done;
  uint64_t ns[4] = {0, 0, 0, 0};
  uint64_t chunks = 0;
  hipEvent_t take() {
    std::lock_guard<std::mutex> lk(mu);
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) e = nullptr;
    return e;
  }
  void give(hipEvent_t e) {
    if (!e) return;
    std::lock_guard<std::mutex> lk(mu);
    pool.push_back(e);
  }
  // completed chunks -> sums.  A chunk another thread enqueued after the
  // caller's synchronisation is left in `done` until its last event has
  // completed (hipEventQuery), so it is neither dropped nor recycled early.
  void collect() {
    std::lock_guard<std::mutex> lk(mu);
    std::vector<std::array<hipEvent_t, 5>> pending;
    for (auto& c : done) {
      if (hipEventQuery(c[4]) == hipErrorNotReady) {
        pending.push_back(c);
        continue;
      }
      uint64_t t[4];
      bool ok = true;
      for (int i = 0; i < 4 && ok; ++i) {
        float ms = 0.f;
        ok = hipEventElapsedTime(&ms, c[i], c[i + 1]) == hipSuccess;
        t[i] = (uint64_t)((double)ms * 1e6);
      }
      if (ok) {
        for (int i = 0; i < 4; ++i) ns[i] += t[i];
        ++chunks;
      }
      for (hipEvent_t e : c) pool.push_back(e);
    }
    done.swap(pending);
  }
  void reset() {
    collect();
    std::lock_guard<std::mutex> lk(mu);
    for (auto& v : ns) v = 0;
    chunks = 0;
  }
  void release() {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& c : done)
      for (hipEvent_t e : c) pool.push_back(e);
    done.clear();
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    pool.clear();
  }
};

// The verify workspace of one stream: every launch that runs kernels on a
// stream uses that stream's workspace, in stream order -- the caller's streams
// (device-resident API) and the library's own pool streams alike, so a pool
// stream shared by several callers and both APIs needs only one.  `mu` is
// held while a launch is planned and enqueued (the workspace may grow), and
// every buffer below is only grown or read under it (the hash
// queue of a shared pool stream was grown outside it).  Caller streams'
// contexts are capped per device (kMaxCallerStreams, least recently used
// evicted) and stl_release_stream drops one: a context lives on in a
// shared_ptr until its last user returns, then hands its buffers to the
// device's spare list (CtxSpares) instead of freeing them.  Every use of a
// caller context ends by recording `done` on its stream (stream_ctx's use
// token), so a spare's buffers are free once `done` has completed: the next
// caller context adopts them and makes its stream wait for that event on the
// device -- no host wait, no hipFree (which would synchronise the whole
// device: VERDICT r5 #4).
// Buffers of the keyset calls that take public keys (stl_keyset_*_by_key*), one
// set per stream context.  A call takes the set out of its context for its
// whole run (ByKeyLease) -- it enqueues through run_verify, which locks the
// contexts itself, so it cannot hold the context's mutex to keep a concurrent
// call on the same stream from growing (freeing) them under its kernels.
struct ByKeyBufs {
  DevBuf idx;    // 256 B of counters ([0]: the miss count), key_index (4 B per row), the miss list (4 B per row)
  DevBuf rows;   // per miss: sig 64 B, msg 32 B, pk 32 B, compact; then their bitmap words
  DevBuf blob;   // the blob form's verify inputs, 128 B per row (as StreamCtx::scratch)
  uint32_t* count = nullptr;  // host-mapped word the miss count is copied to
  hipEvent_t counted = nullptr;  // ... and the event behind that copy
  bool holds() const { return idx.p || rows.p || blob.p || count || counted; }
  void release() {
    idx.release();
    rows.release();
    blob.release();
    if (count) (void)hipHostFree(count);
    count = nullptr;
    if (counted) (void)hipEventDestroy(counted);
    counted = nullptr;
  }
};

struct StreamCtx;
struct CtxSpares {
  std::mutex mu;
  std::vector<std::unique_ptr<StreamCtx>> list;  // oldest first
};
std::atomic<int>& max_caller_streams();
struct StreamCtx {
  std::mutex mu;
  int ordinal = -1;        // device of the buffers below
  bool pool = false;       // a library pool stream's context (never evicted)
  uint64_t last_use = 0;   // LRU tick (Device::ws_mu)
  // caller contexts: completes after the last work enqueued with this
  // context's buffers (recorded on the caller's stream after every use)
  hipEvent_t done = nullptr;
  std::weak_ptr<CtxSpares> spares;  // where the buffers go when the context dies
  DevBuf ws;
  // work counter + longest-first order of the device-resident hash kernels
  // (stl::hash_queue_bytes(n)) of the launches on this stream
  DevBuf queue;
  // fork / join events of launches whose chunks this (caller) stream spreads
  // over pool streams
  hipEvent_t fork = nullptr;
  hipEvent_t join[stl::kMaxVerifyStreams] = {};
  // a launch's shared key domain is built (stl::VerifyExec::key_ready); the
  // one-call blob path's two parse kernels are done (the keys are out)
  hipEvent_t keys = nullptr;
  hipEvent_t parsed[2] = {};
  // R decoded ahead for the one-call checkSign's shared key domain
  // (stl::VerifyExec::rdec: 80 B per row) and its ready event
  DevBuf rdec;
  hipEvent_t rready = nullptr;
  // device-resident automatic dedup: host-mapped word the key sample kernel
  // writes after each call on this stream (1 = its keys repeated); the next
  // call reads it without waiting (feedback, so a stale value only picks the
  // other path -- the bits are the same)
  uint32_t* auto_flag = nullptr;
  uint32_t* auto_flag_dev = nullptr;
  // the device-resident checkSign calls' verify inputs (signing hashes, and
  // from blobs the signatures and keys), 32 or 128 B per row
  DevBuf scratch;
  // the by-key keyset calls' buffers (empty while a call has them out)
  ByKeyBufs bykey;
  // stl_shamap_root_device's workspace (stl::shamap_workspace_bytes)
  DevBuf shamap;
  void release() {
    if (auto_flag) (void)hipHostFree(auto_flag);
    auto_flag = auto_flag_dev = nullptr;
    bykey.release();
    shamap.release();
    scratch.release();
    ws.release();
    queue.release();
    for (hipEvent_t& e : join) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
    if (fork) (void)hipEventDestroy(fork);
    fork = nullptr;
    if (keys) (void)hipEventDestroy(keys);
    keys = nullptr;
    for (hipEvent_t& e : parsed) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
    rdec.release();
    if (rready) (void)hipEventDestroy(rready);
    rready = nullptr;
    if (done) (void)hipEventDestroy(done);
    done = nullptr;
  }
  bool holds_memory() const {
    return auto_flag || scratch.p || ws.p || queue.p || fork || keys || parsed[0] || parsed[1] || rdec.p || rready ||
           done || bykey.holds() || shamap.p;
  }
  // moves every buffer and event of `o` into this (empty) context
  void adopt(StreamCtx& o) {
    std::swap(ws, o.ws);
    std::swap(queue, o.queue);
    std::swap(scratch, o.scratch);
    std::swap(bykey, o.bykey);
    std::swap(shamap, o.shamap);
    std::swap(fork, o.fork);
    std::swap(keys, o.keys);
    std::swap(parsed[0], o.parsed[0]);
    std::swap(parsed[1], o.parsed[1]);
    std::swap(rdec, o.rdec);
    std::swap(rready, o.rready);
    for (uint32_t j = 0; j < stl::kMaxVerifyStreams; ++j) std::swap(join[j], o.join[j]);
    std::swap(auto_flag, o.auto_flag);
    std::swap(auto_flag_dev, o.auto_flag_dev);
    std::swap(done, o.done);
  }
  ~StreamCtx() {
    if (!holds_memory() || ordinal < 0) return;
    // an evicted or released caller context: its buffers go to the device's
    // spares, to be adopted behind `done` (see above), while the list holds
    // fewer than the caller-stream cap
    if (done) {
      if (std::shared_ptr<CtxSpares> sp = spares.lock()) {
        auto z = std::make_unique<StreamCtx>();
        z->ordinal = ordinal;
        z->adopt(*this);
        std::unique_ptr<StreamCtx> over;
        {
          std::lock_guard<std::mutex> lk(sp->mu);
          sp->list.push_back(std::move(z));
          if (sp->list.size() > (size_t)max_caller_streams().load()) {
            over = std::move(sp->list.front());
            sp->list.erase(sp->list.begin());
          }
        }
        return;  // `over` (a spare beyond the cap: no spares link) is freed below
      }
    }
    // no spare list (library shut down, or no `done` event): the buffers'
    // kernels (and the key sample's write to auto_flag) may still be in
    // flight on a stream the caller may have destroyed since, so wait for the
    // whole device before freeing
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (hipSetDevice(ordinal) == hipSuccess) (void)hipDeviceSynchronize();
    release();
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Streams ("stream pool"): HIP maps the streams of a
// process onto GPU_MAX_HW_QUEUES (4 on the pool) hardware queues in creation
// order, and two streams on one queue run one after another.  So libstl makes
// exactly three streams per device, in stl_init, in a fixed order -- two
// kernel streams and one copy stream -- and both APIs share them: the host
// batch API runs even / odd chunks on `stream` / `stream2` and copies on
// `copy`; a device-resident call runs its chunks on the caller's stream plus
// `stream2` (then `stream`).  Made before the caller's later streams, they
// keep their own queues whatever the caller creates afterwards.
void phase_mark(void* ctx, hipStream_t s, int i);  // a PhaseTimer's mark (stl::PhaseClock)
struct Device {
  int ordinal = 0;
  int cus = 0;
  uint32_t grid = 0;  // resident workgroups for the verify kernel
  hipStream_t stream = nullptr;   // kernel stream 0: host batch API even chunks and results
  hipStream_t stream2 = nullptr;  // kernel stream 1: host API odd chunks; a device call's second stream
  hipStream_t copy = nullptr;     // host-to-device copies (overlap the previous chunk's kernels)
  // a device call's fourth stream (STL_TUNE_STREAMS 4 only; made on use under
  // ws_mu, read without a lock by drain / run_verify -- ADVICE r4)
  std::atomic<hipStream_t> stream3{nullptr};
  ncclComm_t comm = nullptr;      // in-process communicator (rank = device index)
  std::mutex mu;
  DevBuf sig, msg, pk, bitmap, pre, off, len, ctr, ctr2, txid, status, wide, gather;
  DevBuf counters;  // device u64 counters of stl_get_stats: [0] accepted, [1] full-length lanes,
                    // [2] / [3] key-cache hits / misses
  // the decoded-key cache (stl_keycache.h): allocated and zeroed once, in
  // setup_device (never lazily: a call's memory use stays flat)
  DevBuf key_cache;
  int key_cache_log2 = 0;  // log2 of its sets; 0: none
  // workspace of every stream used: the pool streams' for good, at most
  // kMaxCallerStreams caller streams' (LRU)
  std::map<hipStream_t, std::shared_ptr<StreamCtx>> stream_ws;
  // buffers of evicted / released caller contexts, adopted by the next ones
  std::shared_ptr<CtxSpares> spares = std::make_shared<CtxSpares>();
  uint64_t ws_tick = 0;
  std::mutex ws_mu;
  void* stage = nullptr;  // pinned host staging of small host batches (run_small), under mu
  size_t stage_cap = 0;
  PhaseTimer timer;
  stl::PhaseClock clock{phase_mark, &timer};
};

// The devices of stl_init, in order (g_mu; read without it after ensure_init).
extern std::vector<std::unique_ptr<Device>> g_devs;

int ensure_init();
// The calling thread's current device, if it is one of g_devs: else STL_ENODEV.
int device_for_call(Device** out);
std::shared_ptr<StreamCtx> stream_ctx(Device& d, hipStream_t s);
int ctx_queue(StreamCtx& c, size_t n, uint32_t** qws, bool blob = false);
uint32_t hash_grid(const Device& d);
uint32_t hash_long_min(const Device& d, size_t n);
unsigned long long* dev_counters(Device& d);
const stl::PhaseClock* phase_clock(Device& d);  // the device's phase clock when timing is on, else none
int check_flags(uint32_t flags);
// the accept predicate's bits alone: what a keyset call or a cache may be given
inline int check_keyset_flags(uint32_t flags) {
  return (flags & ~(STL_POLICY_MASK | STL_REQUIRE_S_LT_L | STL_DEBUG_RAW_PREDICATE)) ? STL_EINVAL : STL_OK;
}
// STL_TUNE_SHAMAP_LOOKUP_BUCKETS: 1 (default) a tree lookup bisects the key's bucket, 0 the whole array
std::atomic<int>& tune_lookup_buckets();
uint64_t now_ns();

// Counts one host entry-point call: signatures, wall time, errors; with
// STL_TRACE=1 one JSON line per call on stderr (host spans; the kernels are
// rocprofv3's).
struct CallSpan {
  const char* name;
  size_t n;
  uint64_t t0 = now_ns();
  int finish(int rc, uint64_t gather_ns = 0);
};

// Restores the calling thread's current HIP device on scope exit: the host
// entry points switch devices internally, and a library call must not leave
// the caller (stellard, or a PyTorch user of the device API) on another one.
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// ---- live handle objects (keysets, account directories, verified-ID caches) ----
// Every LiveSet, so that stl_shutdown releases them all without naming them.
struct LiveSetBase {
  LiveSetBase* const next;
  LiveSetBase() : next(head) { head = this; }
  virtual void release_all() = 0;
  static void release_every() { for (LiveSetBase* s = head; s; s = s->next) s->release_all(); }
  static LiveSetBase* head;  // constant-initialised: null before the first LiveSet is constructed
};

// Which of for_call's two answers comes first when both apply.
enum class CheckFirst {
  kHandle,  // a dead handle is STL_EINVAL even where the thread has no device (keysets)
  kDevice,  // without a device STL_ENODEV comes before the handle is looked at (directories, caches)
};

// The live objects of one handle type T, which supplies `ordinal` (its
// device) and release() of its DevBufs.  `mu` is held while a call looks its
// handle up and enqueues the kernels that touch the object, and while an
// object is destroyed -- so a handle that passed the lookup stays alive until
// its work is on the stream, and destroy (which then waits for the device)
// sees all of it.  Lock order: a LiveSet's mu before g_mu, before a device's
// mu, before a stream context's mu.  live() and for_call() want mu held;
// add(), destroy() and release_all() take it.
template <typename T, CheckFirst first>
struct LiveSet final : LiveSetBase {
  std::mutex mu;
  bool live(const T* h) const { return h && set_.count(h); }
  // The live object of a handle on the calling thread's device.
  int for_call(const T* h, Device** d) const {
    if (first == CheckFirst::kHandle && !live(h)) return STL_EINVAL;
    STL_RC(device_for_call(d));
    if (!live(h)) return STL_EINVAL;
    return (*d)->ordinal == h->ordinal ? STL_OK : STL_EINVAL;
  }
  void add(T* h) {
    std::lock_guard<std::mutex> lk(mu);
    set_.insert(h);
  }
  void destroy(T* h) {
    std::lock_guard<std::mutex> lk(mu);
    if (live(h)) free_locked(h);
  }
  void release_all() override {
    std::lock_guard<std::mutex> lk(mu);
    while (!set_.empty()) free_locked(const_cast<T*>(*set_.begin()));
  }

 private:
  std::set<const T*> set_;
  // Waits for the device, then frees the object.
  void free_locked(T* h) {
    set_.erase(h);
    DeviceGuard guard;
    if (hipSetDevice(h->ordinal) == hipSuccess) (void)hipDeviceSynchronize();
    h->release();
    delete h;
  }
};

// ---- one synchronous host call on one device ----
// From "arguments checked, device chosen" to "outputs copied, span finished":
// holds the device's mutex and restores the thread's device.  run() makes the
// device current and calls the body, which uploads (rows, upload), enqueues
// its kernels on d.stream and names its outputs (download); these come back
// through one bounce buffer behind one hipStreamSynchronize.  On any failure
// the stream is idle before run() returns and the caller's arrays are untouched.
struct HostCall {
  CallSpan span;
  DeviceGuard guard;
  Device& d;
  std::lock_guard<std::mutex> dl;
  HostCall(const char* name, size_t n, Device& dev) : span{name, n}, d(dev), dl(dev.mu) {}
  // Variable-length rows -> d.pre / d.off / d.len, rebased on their lowest offset.
  int rows(const uint8_t* bytes, const uint64_t* off, const uint32_t* len, size_t n);
  // `bytes` of src -> b, grown first.
  int upload(DevBuf& b, const void* src, size_t bytes);
  // dst <- the first `bytes` of b, once everything has succeeded; no dst, no copy.
  void download(void* dst, const DevBuf& b, size_t bytes) { if (dst) outs_.push_back(Out{dst, &b, bytes}); }
  int run(const std::function<int()>& body);

 private:
  struct Out { void* dst; const DevBuf* b; size_t bytes; };
  int fetch();
  std::vector<uint64_t> roff_, row_end_;  // sources of asynchronous copies: they live as long as the call
  std::vector<Out> outs_;
  std::vector<uint8_t> bounce_;
};

// ---- verify by public key ----
// One call's hold on its stream context's by-key buffers: taken out of the
// context under its mutex, put back the same way.  Should a concurrent call on
// the same stream have put its own set back first, the larger of the two stays
// and the other is freed once the stream has drained.
struct ByKeyLease {
  std::shared_ptr<StreamCtx> c;
  hipStream_t s;
  ByKeyBufs b;
  ByKeyLease(std::shared_ptr<StreamCtx> ctx, hipStream_t stream) : c(std::move(ctx)), s(stream) {
    std::lock_guard<std::mutex> lk(c->mu);
    std::swap(b, c->bykey);
  }
  ~ByKeyLease() {
    {
      std::lock_guard<std::mutex> lk(c->mu);
      if (b.idx.cap + b.rows.cap + b.blob.cap >= c->bykey.idx.cap + c->bykey.rows.cap + c->bykey.blob.cap)
        std::swap(b, c->bykey);
    }
    if (!b.holds()) return;
    (void)hipStreamSynchronize(s);
    b.release();
  }
  ByKeyLease(const ByKeyLease&) = delete;
  ByKeyLease& operator=(const ByKeyLease&) = delete;
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- the miss path: calls that decide most rows from a table (the keyset by
// key, the verified-ID cache) and send the rest through the general verify.
// None of these takes a registry mutex: where a caller releases and retakes
// its own stays in the caller.
// The serialized-object pass of stl_signed_blob_prepare_device on stream s,
// with context c's queue under c's mutex until the kernel is enqueued.
int blob_prepare(Device& d, StreamCtx& c, uint32_t kind, const uint8_t* d_blobs, const uint64_t* d_offset,
                 const uint32_t* d_len, size_t n, uint8_t* d_msg, uint8_t* d_sig, uint8_t* d_pk, uint8_t* d_id,
                 uint8_t* d_status, hipStream_t s);
// b.idx of idx_bytes, and on first use the host-mapped words the counts are
// copied to and the event behind that copy.
int miss_counters(ByKeyBufs& b, size_t idx_bytes);
// Rows miss_rows[0 .. m) of sig / msg / pk, compacted into use.b.rows, through
// run_verify as stl_ed25519_verify_batch_device runs them (the key dedup left
// to the stream's automatic choice, sampled on the compact keys: signers
// outside a keyset repeat as well); their bits are ORed into d_words.
// *compact_words: the m rows' own bitmap.
int verify_misses(Device& d, ByKeyLease& use, const uint32_t* miss_rows, size_t m, const uint8_t* d_sig,
                  const uint8_t* d_msg, const uint8_t* d_pk, uint64_t* d_words, uint32_t flags, hipStream_t s,
                  const uint64_t** compact_words = nullptr);

}  // namespace stl
