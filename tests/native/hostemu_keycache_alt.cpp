// hostemu_keycache_alt.cpp -- TEST HARNESS ONLY.  The decoded-key cache's
// second-choice set (stellard_amd/csrc/stl_keycache.h: key_cache_alt_set and
// the insert rule key_cache_place) and phase 1's point half split in two
// (stl_verify_core.h: verify_phase1_points_r, then finish_phase1_points), as
// the gfx950 kernels run them, for the CPU test suite.  Limb bounds are
// checked as in hostemu.cpp.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

static std::atomic<uint64_t> g_bound_viol{0};

#define STL_BOUND_MUL(a, b) kca_check_mul((a), (b))
#define STL_BOUND_SUB(a, b) kca_check_sub((a), (b))
#define STL_BOUND_SUBK(a, b, K) kca_check_subk((a), (b), (K))
namespace stl { struct fe; }
static void kca_check_mul(const stl::fe& a, const stl::fe& b);
static void kca_check_sub(const stl::fe& a, const stl::fe& b);
static void kca_check_subk(const stl::fe& a, const stl::fe& b, int k);

#include "../../stellard_amd/csrc/stl_verify_core.h"
#include "../../stellard_amd/csrc/stl_keycache.h"

static double alpha(const stl::fe& a) {
  uint32_t m = 0;
  for (int i = 0; i < 9; ++i) m = a.v[i] > m ? a.v[i] : m;
  return m / 536870912.0;
}
static void kca_check_mul(const stl::fe& a, const stl::fe& b) {
  if (alpha(a) * alpha(b) > 7.0) g_bound_viol++;
}
static void kca_check_sub(const stl::fe& a, const stl::fe& b) {
  if (alpha(a) > 3.9 || alpha(b) > 3.9) g_bound_viol++;
}
static void kca_check_subk(const stl::fe& a, const stl::fe& b, int k) {
  bool bad = b.v[0] > (uint64_t)k * 0x1ffffb40u;
  for (int i = 1; i < 9; ++i) bad = bad || b.v[i] > (uint64_t)k * 0x1fffffffu;
  for (int i = 0; i < 9; ++i) bad = bad || (uint64_t)a.v[i] + (uint64_t)k * 0x1fffffffu > 0xffffffffull;
  if (bad) g_bound_viol++;
}

namespace {

struct Bits {
  uint32_t same, empty;
};
// what an insert sees of one set of a tag-only model: bit w of same / empty
Bits look(const uint64_t* tags, const uint8_t* used, uint32_t set, uint64_t tag) {
  Bits b{0, 0};
  for (uint32_t w = 0; w < stl::kKeyCacheWays; ++w) {
    const size_t s = (size_t)set * stl::kKeyCacheWays + w;
    if (!used[s]) b.empty |= 1u << w;
    else if (tags[s] == tag) b.same |= 1u << w;
  }
  return b;
}

}  // namespace

extern "C" {

uint64_t hostemu_kca_bound_violations(void) { return g_bound_viol.load(); }

// primary and alternate set of n keys under `mask`
void hostemu_kca_index(const uint8_t* keys, size_t n, uint32_t mask, uint32_t* set, uint32_t* alt) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t A[8];
    std::memcpy(A, keys + 32 * i, 32);
    set[i] = stl::key_cache_set(stl::key_hash(A), mask);
    alt[i] = stl::key_cache_alt_set(A, mask);
  }
}

// key_cache_place on n patterns: bit w of same0 / empty0 (primary set) and
// same1 / empty1 (alternate set); the hash is one whose first way is
// first_way[i].  out[i] = way | 8 if the alternate set is written.
void hostemu_kca_place(size_t n, const uint32_t* first_way, const uint32_t* same0, const uint32_t* empty0,
                       const uint32_t* same1, const uint32_t* empty1, uint32_t* out) {
  uint32_t top_of[stl::kKeyCacheWays];
  for (uint32_t top = 256; top-- > 0;) top_of[stl::key_cache_first_way(top << 24)] = top;
  for (size_t i = 0; i < n; ++i) {
    bool alt = false;
    const uint32_t w = stl::key_cache_place(top_of[first_way[i]] << 24, same0[i], empty0[i], same1[i], empty1[i], alt);
    out[i] = w | (alt ? 8u : 0u);
  }
}

// Sequential insertion of n keys into 2^log2_sets sets of tags under the
// insert rule, each with the real key_hash, tag and alternate set.  out[0] =
// inserts that found neither set with the key's tag or an empty way (they
// overwrote another key), out[1] = keys written to their alternate set,
// out[2] = keys a lookup (primary set's tags, then the alternate set's) does
// not find once all are in.
void hostemu_kca_fill(const uint8_t* keys, size_t n, uint32_t log2_sets, uint64_t out[3]) {
  const uint32_t mask = (1u << log2_sets) - 1u;
  const size_t slots = ((size_t)mask + 1) * stl::kKeyCacheWays;
  std::vector<uint64_t> tags(slots, 0);
  std::vector<uint8_t> used(slots, 0);
  out[0] = out[1] = out[2] = 0;
  auto ident = [&](size_t i, uint32_t& h, uint32_t& s0, uint32_t& s1, uint64_t& tag) {
    uint32_t A[8], t[2];
    std::memcpy(A, keys + 32 * i, 32);
    h = stl::key_hash(A);
    s0 = stl::key_cache_set(h, mask);
    s1 = stl::key_cache_alt_set(A, mask);
    stl::key_cache_tag(t, A);
    tag = (uint64_t)t[1] << 32 | t[0];
  };
  for (size_t i = 0; i < n; ++i) {
    uint32_t h, s0, s1;
    uint64_t tag;
    ident(i, h, s0, s1, tag);
    const Bits b0 = look(tags.data(), used.data(), s0, tag), b1 = look(tags.data(), used.data(), s1, tag);
    if (!(b0.same | b0.empty | b1.same | b1.empty)) out[0]++;
    bool alt = false;
    const uint32_t w = stl::key_cache_place(h, b0.same, b0.empty, b1.same, b1.empty, alt);
    out[1] += alt;
    const size_t s = (size_t)(alt ? s1 : s0) * stl::kKeyCacheWays + w;
    tags[s] = tag;
    used[s] = 1;
  }
  for (size_t i = 0; i < n; ++i) {
    uint32_t h, s0, s1;
    uint64_t tag;
    ident(i, h, s0, s1, tag);
    if (!look(tags.data(), used.data(), s0, tag).same && !look(tags.data(), used.data(), s1, tag).same) out[2]++;
  }
}

// n rows: the scalar half, then (a) verify_phase1_points, (b) the R half,
// A's decoding and finish_phase1_points.  Both 224-byte states per row;
// returns the rows whose two states differ.
uint64_t hostemu_kca_split(const uint8_t* sig, const uint8_t* msg, const uint8_t* pk, size_t n, uint32_t policy,
                           uint8_t* whole, uint8_t* split) {
  uint64_t differ = 0;
  for (size_t i = 0; i < n; ++i) {
    uint32_t R[8], S[8], A[8], M[8], h[16], k[8];
    std::memcpy(R, sig + 64 * i, 32);
    std::memcpy(S, sig + 64 * i + 32, 32);
    std::memcpy(A, pk + 32 * i, 32);
    std::memcpy(M, msg + 32 * i, 32);
    stl::sha512_hram32(h, R, A, M);
    stl::sc_reduce64(k, h);
    stl::HalfState a, b;
    std::memset(&a, 0, sizeof a);
    std::memset(&b, 0, sizeof b);
    stl::verify_phase1_scalars(a, S, k);
    stl::verify_phase1_scalars(b, S, k);
    stl::verify_phase1_points(a, R, S, A, policy);
    stl::fe nQx, nQy;
    const bool okr = stl::verify_phase1_points_r(nQx, nQy, R, S, A, policy);
    stl::ge_p3 negA;
    const bool okA = stl::ge_frombytes_negate_vartime(negA, A);
    stl::finish_phase1_points(b, negA.X, negA.Y, nQx, nQy, okr && okA);
    std::memcpy(whole + 224 * i, &a, 224);
    std::memcpy(split + 224 * i, &b, 224);
    differ += std::memcmp(&a, &b, 224) != 0;
  }
  return differ;
}

}  // extern "C"
