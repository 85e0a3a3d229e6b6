// hostemu_keycache.cpp -- TEST HARNESS ONLY.  The decoded-key cache's host-
// compilable parts (stellard_amd/csrc/stl_keycache.h: the check that guards
// every x read from the cache, the set / way hash and the victim choice, as
// the gfx950 kernels run them) and the verify workspace's layout function
// (stl_kernels.h), for the CPU test suite.  Limb bounds are checked as in
// hostemu.cpp.
#include <atomic>
#include <cstdint>
#include <cstring>

static std::atomic<uint64_t> g_bound_viol{0};

#define STL_BOUND_MUL(a, b) kc_check_mul((a), (b))
#define STL_BOUND_SUB(a, b) kc_check_sub((a), (b))
#define STL_BOUND_SUBK(a, b, K) kc_check_subk((a), (b), (K))
namespace stl { struct fe; }
static void kc_check_mul(const stl::fe& a, const stl::fe& b);
static void kc_check_sub(const stl::fe& a, const stl::fe& b);
static void kc_check_subk(const stl::fe& a, const stl::fe& b, int k);

#include "../../stellard_amd/csrc/stl_ge25519.h"
#include "../../stellard_amd/csrc/stl_keycache.h"
#include "../../stellard_amd/csrc/stl_kernels.h"

static double alpha(const stl::fe& a) {
  uint32_t m = 0;
  for (int i = 0; i < 9; ++i) m = a.v[i] > m ? a.v[i] : m;
  return m / 536870912.0;
}
static void kc_check_mul(const stl::fe& a, const stl::fe& b) {
  if (alpha(a) * alpha(b) > 7.0) g_bound_viol++;
}
static void kc_check_sub(const stl::fe& a, const stl::fe& b) {
  if (alpha(a) > 3.9 || alpha(b) > 3.9) g_bound_viol++;
}
static void kc_check_subk(const stl::fe& a, const stl::fe& b, int k) {
  bool bad = b.v[0] > (uint64_t)k * 0x1ffffb40u;
  for (int i = 1; i < 9; ++i) bad = bad || b.v[i] > (uint64_t)k * 0x1fffffffu;
  for (int i = 0; i < 9; ++i) bad = bad || (uint64_t)a.v[i] + (uint64_t)k * 0x1fffffffu > 0xffffffffull;
  if (bad) g_bound_viol++;
}

extern "C" {

uint64_t hostemu_kc_bound_violations(void) { return g_bound_viol.load(); }

// out: default / smallest / largest log2 of the sets, ways, bytes per set, and
// inside a set the byte offset of way 0's tag (8 B each) and x (32 B each)
void hostemu_kc_geometry(uint32_t out[7]) {
  out[0] = (uint32_t)stl::kKeyCacheLog2Default;
  out[1] = (uint32_t)stl::kKeyCacheLog2Min;
  out[2] = (uint32_t)stl::kKeyCacheLog2Max;
  out[3] = stl::kKeyCacheWays;
  out[4] = stl::kKeyCacheSetBytes;
  out[5] = stl::kKeyCacheTagWord * 4;
  out[6] = stl::kKeyCacheXWord * 4;
}

// The decoder on n keys: ok[i], and the canonical bytes of x(-A).
void hostemu_kc_decode(const uint8_t* keys, size_t n, uint8_t* xbytes, uint8_t* ok) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t A[8], xb[8];
    std::memcpy(A, keys + 32 * i, 32);
    stl::ge_p3 negA;
    ok[i] = stl::ge_frombytes_negate_vartime(negA, A) ? 1 : 0;
    stl::fe_tobytes(xb, negA.X);
    std::memcpy(xbytes + 32 * i, xb, 32);
  }
}

// key_cache_certify on n (key, candidate) pairs: pass[i], and fe_tobytes of the X it returned.
void hostemu_kc_certify(const uint8_t* keys, const uint8_t* cand, size_t n, uint8_t* pass, uint8_t* xcanon) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t A[8], xb[8], out[8];
    std::memcpy(A, keys + 32 * i, 32);
    std::memcpy(xb, cand + 32 * i, 32);
    stl::fe X;
    pass[i] = stl::key_cache_certify(X, A, xb) ? 1 : 0;
    stl::fe_tobytes(out, X);
    std::memcpy(xcanon + 32 * i, out, 32);
  }
}

// set index under `mask`, first way and tag (2 words each) of n keys
void hostemu_kc_index(const uint8_t* keys, size_t n, uint32_t mask, uint32_t* set, uint32_t* way, uint32_t* tag) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t A[8];
    std::memcpy(A, keys + 32 * i, 32);
    const uint32_t h = stl::key_hash(A);
    set[i] = stl::key_cache_set(h, mask);
    way[i] = stl::key_cache_first_way(h);
    stl::key_cache_tag(tag + 2 * i, A);
  }
}

// bit w of same_bits / empty_bits: way w holds the key's tag / is all zero;
// the hash is one whose first way is first_way
uint32_t hostemu_kc_victim(uint32_t first_way, uint32_t same_bits, uint32_t empty_bits) {
  bool same[stl::kKeyCacheWays], empty[stl::kKeyCacheWays];
  for (uint32_t w = 0; w < stl::kKeyCacheWays; ++w) {
    same[w] = (same_bits >> w) & 1u;
    empty[w] = (empty_bits >> w) & 1u;
  }
  for (uint32_t top = 0; top < 256; ++top)
    if (stl::key_cache_first_way(top << 24) == first_way) return stl::key_cache_victim(top << 24, same, empty);
  return 0xFFFFFFFFu;  // no such way
}

// The workspace's sub-buffers for a launch grid: offsets from verify_ws_layout,
// sizes as the kernels use them (stated here, not derived from the layout).
// Order: slots, pre, fb, queue, miss, miss_ctr, then the key domain's kslots,
// rep, uid_of, owners, counter, keytab, keytabs, widetabs.  Returns their
// number; total[0] / total[1] = verify_ws_bytes(grid, false / true).
uint32_t hostemu_ws_layout(uint32_t grid, uint64_t* off, uint64_t* size, uint64_t total[2]) {
  const stl::VerifyWsLayout l = stl::verify_ws_layout(grid);
  const uint64_t o[14] = {l.slots, l.pre, l.fb, l.queue, l.miss, l.miss_ctr, l.kslots,
                          l.rep, l.uid_of, l.owners, l.counter, l.keytab, l.keytabs, l.widetabs};
  const uint64_t s[14] = {(uint64_t)grid * stl::kBlock * stl::kSlotQuads * 16,
                          (uint64_t)stl::kPreChunk * 224,
                          (uint64_t)stl::kPreChunk / 8,
                          (uint64_t)stl::kMainQueueWords * 4,
                          (uint64_t)stl::kPreChunk * 4,
                          (uint64_t)stl::kMainQueueWords * 4,
                          (uint64_t)stl::kDedupSlots * 4,
                          (uint64_t)stl::kPreChunk * 4,
                          (uint64_t)stl::kPreChunk * 4,
                          (uint64_t)stl::kPreChunk * 4,
                          4,
                          (uint64_t)stl::kPreChunk * 5 * 16,
                          (uint64_t)stl::kKeyTables * 81 * 16,
                          (uint64_t)stl::kWideKeys * 137 * 9 * 16};
  for (int i = 0; i < 14; ++i) {
    off[i] = o[i];
    size[i] = s[i];
  }
  total[0] = stl::verify_ws_bytes(grid, false);
  total[1] = stl::verify_ws_bytes(grid, true);
  return 14;
}

}  // extern "C"
