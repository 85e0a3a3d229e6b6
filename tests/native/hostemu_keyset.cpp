// hostemu_keyset.cpp -- TEST HARNESS ONLY.  Compiles the keyset's device code
// (stellard_amd/csrc/stl_comb.h, the exact functions the gfx950 kernels of
// stl_keyset.hip run) for the host, with the limb-bound hooks of hostemu.cpp,
// so that the comb tables and the doubling-free verify can be checked against
// independent arithmetic and the oracle in the CPU test suite.  Not part of
// the product library (libstl exposes no CPU verify path).
#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

static std::atomic<uint64_t> g_bound_viol{0};
static std::atomic<uint64_t> g_bound_checks{0};

#define STL_BOUND_MUL(a, b) hostemu_check_mul((a), (b))
#define STL_BOUND_SUB(a, b) hostemu_check_sub((a), (b))
#define STL_BOUND_SUBK(a, b, K) hostemu_check_subk((a), (b), (K))
namespace stl { struct fe; }
static void hostemu_check_mul(const stl::fe& a, const stl::fe& b);
static void hostemu_check_sub(const stl::fe& a, const stl::fe& b);
static void hostemu_check_subk(const stl::fe& a, const stl::fe& b, int k);

#include "../../stellard_amd/csrc/stl_comb.h"

static double alpha(const stl::fe& a) {
  uint32_t m = 0;
  for (int i = 0; i < 9; ++i) m = a.v[i] > m ? a.v[i] : m;
  return m / 536870912.0;
}
static void hostemu_check_mul(const stl::fe& a, const stl::fe& b) {
  g_bound_checks++;
  if (alpha(a) * alpha(b) > 7.0) g_bound_viol++;
}
// fe_sub_nc<K>: no limb of b above K*Z1's, and a + K*Z1 within 32 bits
static void hostemu_check_subk(const stl::fe& a, const stl::fe& b, int k) {
  g_bound_checks++;
  bool bad = b.v[0] > (uint64_t)k * 0x1ffffb40u;
  for (int i = 1; i < 9; ++i) bad = bad || b.v[i] > (uint64_t)k * 0x1fffffffu;
  for (int i = 0; i < 9; ++i) bad = bad || (uint64_t)a.v[i] + (uint64_t)k * 0x1fffffffu > 0xffffffffull;
  if (bad) g_bound_viol++;
}
static void hostemu_check_sub(const stl::fe& a, const stl::fe& b) {
  g_bound_checks++;
  if (alpha(a) > 3.9 || alpha(b) > 3.9) g_bound_viol++;
}

static void load8(uint32_t w[8], const uint8_t* p) { std::memcpy(w, p, 32); }

// B's encoding: y = 4/5, x positive
static void base_bytes(uint8_t out[32]) {
  std::memset(out, 0x66, 32);
  out[0] = 0x58;
}

// One window of the table of the key `rec` describes, as keyset_build_kernel
// builds it.
static void build_window(uint32_t* rows, const uint32_t* rec, int w) {
  uint32_t scratch[stl::kCombScratchWords];
  stl::ge_p3 P, W;
  stl::comb_record_point(P, rec);
  stl::comb_window_base(W, P, w);
  stl::comb_build_window(rows, scratch, W);
}

// Record and (when the key decodes) table of a32, or of the base point for
// a32 = nullptr.  table: kCombKeyWords words, zero-filled first (a key that
// does not decode keeps zero rows, as on the device).
static void build_key(uint32_t* rec, uint32_t* table, const uint8_t* a32) {
  uint8_t b[32];
  if (!a32) base_bytes(b);
  uint32_t A[8];
  load8(A, a32 ? a32 : b);
  stl::comb_key_record(rec, A, a32 == nullptr);
  std::memset(table, 0, stl::kCombKeyWords * 4);
  if (rec[stl::kKeyRecFlags] & stl::kKeyDecodes)
    for (int w = 0; w < stl::kCombWindows; ++w)
      build_window(table + (size_t)w * stl::kCombRows * stl::kCombRowWords, rec, w);
}

static const uint32_t* base_table() {
  static std::vector<uint32_t> tab;
  static std::once_flag once;
  std::call_once(once, [] {
    tab.resize(stl::kCombKeyWords);
    uint32_t rec[stl::kKeyRecWords];
    build_key(rec, tab.data(), nullptr);
  });
  return tab.data();
}

extern "C" {

uint64_t hostemu_bound_checks(void) { return g_bound_checks.load(); }
uint64_t hostemu_bound_violations(void) { return g_bound_viol.load(); }

// Table geometry, for tests that must not hard-code it.
void hostemu_keyset_geometry(uint32_t out[4]) {
  out[0] = stl::kCombBits;
  out[1] = stl::kCombWindows;
  out[2] = stl::kCombRows;
  out[3] = stl::kCombRowWords * 4;
}

// A key's whole table (a32 = NULL: the base point's) built with the kernels'
// functions: out_words holds windows * rows * row_bytes / 4 words.  Returns
// the key's flags (stl_comb.h kKey*).
uint32_t hostemu_keyset_table(const uint8_t* a32, uint32_t* out_words) {
  uint32_t rec[stl::kKeyRecWords];
  build_key(rec, out_words, a32);
  return rec[stl::kKeyRecFlags];
}

// Row (w, j), j = 1..rows, of the table of a32 (NULL: the base point).
// Returns 0, or -1 for a key that does not decode (no rows) or a bad (w, j).
int hostemu_comb_row(const uint8_t* a32, uint32_t w, uint32_t j, uint32_t* out_words) {
  if (w >= (uint32_t)stl::kCombWindows || j < 1 || j > (uint32_t)stl::kCombRows) return -1;
  uint8_t b[32];
  if (!a32) base_bytes(b);
  uint32_t A[8], rec[stl::kKeyRecWords];
  load8(A, a32 ? a32 : b);
  stl::comb_key_record(rec, A, a32 == nullptr);
  if (!(rec[stl::kKeyRecFlags] & stl::kKeyDecodes)) return -1;
  std::vector<uint32_t> win((size_t)stl::kCombRows * stl::kCombRowWords);
  build_window(win.data(), rec, (int)w);
  std::memcpy(out_words, &win[(size_t)(j - 1) * stl::kCombRowWords], stl::kCombRowWords * 4);
  return 0;
}

// encode([S]B + [k](-A)) by the comb (S masked to 253 bits, k as given:
// callers pass k < 2^253).  Returns -1 when A does not decode.
int hostemu_comb_point(const uint8_t* k32, const uint8_t* S32, const uint8_t* A32, uint8_t* out32) {
  // the last key's table is kept: a test walks many scalars over one key
  static std::vector<uint32_t> tab(stl::kCombKeyWords);
  static uint32_t rec[stl::kKeyRecWords];
  static uint8_t have[32];
  static bool valid = false;
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (!valid || std::memcmp(have, A32, 32) != 0) {
    build_key(rec, tab.data(), A32);
    std::memcpy(have, A32, 32);
    valid = true;
  }
  if (!(rec[stl::kKeyRecFlags] & stl::kKeyDecodes)) return -1;
  uint32_t k[8], S[8], enc[8];
  load8(k, k32);
  load8(S, S32);
  stl::comb_point_bytes(enc, k, S, tab.data(), base_table(), true);
  std::memcpy(out32, enc, 32);
  return 0;
}

// The same encoding by the Straus loop of the per-signature kernels
// (double_scalarmult + ge_tobytes, S masked as verify_phase2 masks it).
int hostemu_straus_point(const uint8_t* k32, const uint8_t* S32, const uint8_t* A32, uint8_t* out32) {
  uint32_t A[8], k[8], S[8], enc[8];
  load8(A, A32);
  load8(k, k32);
  load8(S, S32);
  S[7] &= 0x1fffffffu;
  stl::ge_p3 negA;
  if (!stl::ge_frombytes_negate_vartime(negA, A)) return -1;
  std::vector<uint4> table(81);
  stl::ge_p2 Rp;
  stl::double_scalarmult(Rp, negA, k, S, stl::TableView::contiguous(table.data()), &stl::kBaseNielsHost[0][0][0]);
  stl::ge_tobytes(enc, Rp);
  std::memcpy(out32, enc, 32);
  return 0;
}

// The keyset verify as keyset_verify_kernel runs it: tables of the nkeys keys
// built on `threads` threads (kept until the next call with other keys), then
// one verify_comb_with_k per row.  Bitmap LSB-first; a key_index >= nkeys
// gives bit 0.  Returns the number of limb-bound violations observed.
uint64_t hostemu_keyset_verify_batch(const uint8_t* pk_set, uint32_t nkeys, const uint32_t* key_index,
                                     const uint8_t* sig, const uint8_t* msg, size_t n, uint8_t* bitmap,
                                     uint32_t policy) {
  static std::vector<uint8_t> have;
  static std::vector<uint32_t> recs, tabs;
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (have.size() != (size_t)nkeys * 32 || std::memcmp(have.data(), pk_set, have.size()) != 0) {
    recs.assign((size_t)nkeys * stl::kKeyRecWords, 0);
    tabs.resize((size_t)nkeys * stl::kCombKeyWords);
    std::vector<std::thread> th;
    const uint32_t T = 8;
    for (uint32_t t = 0; t < T; ++t)
      th.emplace_back([&, t] {
        for (uint32_t i = t; i < nkeys; i += T)
          build_key(&recs[(size_t)i * stl::kKeyRecWords], &tabs[(size_t)i * stl::kCombKeyWords], pk_set + 32 * (size_t)i);
      });
    for (auto& x : th) x.join();
    have.assign(pk_set, pk_set + (size_t)nkeys * 32);
  }
  const uint32_t* base = base_table();
  std::memset(bitmap, 0, (n + 7) / 8);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t ki = key_index[i];
    if (ki >= nkeys) continue;
    const uint32_t* rec = &recs[(size_t)ki * stl::kKeyRecWords];
    uint32_t R[8], S[8], M[8], h[16], k[8];
    load8(R, sig + 64 * i);
    load8(S, sig + 64 * i + 32);
    load8(M, msg + 32 * i);
    stl::sha512_hram32(h, R, rec, M);
    stl::sc_reduce64(k, h);
    if (stl::verify_comb_with_k(R, S, rec[stl::kKeyRecFlags], k, policy, &tabs[(size_t)ki * stl::kCombKeyWords], base))
      bitmap[i >> 3] |= (uint8_t)(1u << (i & 7));
  }
  return g_bound_viol.load();
}

}  // extern "C"
