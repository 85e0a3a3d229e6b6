// stl_sigcache_core.h -- the verified-ID cache (stl_sigcache_*): the IDs of
// signed objects libstl's own verify has accepted, kept on the device from one
// call to the next, so that a row whose ID is found skips the Ed25519 verify.
// The device-resident counterpart of HashRouter's SF_SIGGOOD
// (IHashRouter.h:27-33, HashRouter.cpp:203-222).  Plain C++: the kernels of
// stl_sigcache.hip and the host build of tests/native/hostemu_sigcache.cpp
// compile the same functions.
//
// WHY A HIT IS THE VERDICT.  A transaction's ID is SHA512Half("TXN\0" || blob),
// a validation's SHA512Half(blob): it commits to every byte of the blob, the
// signature and the key included.  A row's status and accept bit are a pure
// function of the blob and the accept predicate, and a cache is bound to one
// kind and one predicate when it is made.  So "this exact ID was accepted
// before by this predicate" is the accept bit; it never goes stale and needs
// no ledger state.  Only accepts are kept, and only libstl's own verify
// inserts them.
//
// WHAT A READER MAY SEE.  Slots are read while other lanes, waves and streams
// write them, with no lock, fence or state word.
//   * Granularity: a naturally aligned 32-bit word is written whole; nothing
//     wider is assumed.  A slot that two inserts overwrite at once (an
//     eviction), or that is read half-way through one insert, may hold any
//     mixture of the 32-bit words of the IDs written to that way, and zeros
//     (a way is claimed by its first 64 bits, the other 24 bytes follow).
//   * Every ID ever written is the ID of a row this cache's predicate
//     accepted.  So a torn or half-written slot equals a row's ID only if
//     that ID is assembled, word for word, from the IDs of accepted rows of
//     the slot's history and zero words.
//   * Such an ID is infeasible: with q IDs in the history of one way there
//     are at most (q + 1)^8 such assemblies among 2^256 outputs, so a trial
//     blob's ID is one of them with probability (q + 1)^8 / 2^256 -- under
//     2^-128 for q < 2^16, per hash evaluation -- and each assembly that is
//     no whole accepted ID needs a second preimage of a 256-bit value that
//     nobody has computed.
//   * Nothing but the equality of all 32 bytes of one way with the row's ID
//     sets a bit: no tags, no partial compares.  The all-zero ID, and any ID
//     whose first 64 bits are zero, never hits and is never stored, so an
//     empty or cleared way matches nothing.
//   * How soon one stream's insert is seen by another, whether an insert
//     survives a racing clear, and which ID an eviction leaves only move the
//     hit rate.  A miss is verified as without a cache.
//
// Geometry.  2^K sets (K = sets_log2, 0..24), each one 128-byte aligned line
// of 4 ways, a way the 32 bytes of an ID:
//     words 8 w .. 8 w + 7   the ID of way w       (w = 0..3)
// An empty way is all zero; a way is empty exactly when its first 64 bits are
// zero.  The set index is bits 32..55 of a seeded 64-bit hash of the ID under
// the set mask, the way an insert starts from its top two bits, which no mask
// uses.
//
// Insert.  Nothing, if the line as read holds the ID.  Otherwise the ways are
// walked from the hash's way with one 64-bit compare-and-swap each on the
// way's first word (0 -> the ID's first word):
//     0 came back          the way is ours: the other 24 bytes are written
//     our first word       another lane is storing this ID there: done
//     anything else        taken: the next way
// and when all four are taken the hash's way is overwritten whole (eviction).
// The walk reads nothing but what the compare-and-swaps return, so it does
// not depend on when another workgroup's plain stores become visible.
// GUARANTEE: while a set has received at most 4 distinct IDs since it was
// made or cleared, all of them are present once the inserting work has
// completed, however many lanes, waves or streams inserted them at once.
// (An ID walks its ways in one fixed order and ways are never freed, so the
// lanes of one ID all end at the same way and an ID takes one way; four IDs
// find four ways.)  It is stated for IDs whose first 64 bits differ pairwise:
// of two IDs that share them -- 2^-64 per pair by chance; 2^32 signed
// transactions ground for it give one pair -- the later may be left out,
// which costs a verify, never a bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

namespace stl {

constexpr uint32_t kScWays = 4;
constexpr uint32_t kScIdWords = 8;                        // an ID: 32 bytes
constexpr uint32_t kScLineWords = kScWays * kScIdWords;   // 128 bytes
constexpr uint32_t kScLog2Max = 24;                       // 2 GiB
static_assert(kScLineWords * 4 == 128, "a set is one 128-byte line");
static_assert(32 + kScLog2Max <= 62, "the way bits lie above every set mask");

// include/stl.h: the flag bits that decide an accept bit (STL_POLICY_MASK |
// STL_DEBUG_RAW_PREDICATE), and the status of a row the verify decides
constexpr uint32_t kScPredicateMask = 0x80000001u;
constexpr uint32_t kScTxOk = 0;

#define STL_SC_HD __host__ __device__ inline

inline size_t sigcache_bytes(uint32_t sets_log2) { return (size_t)(kScLineWords * 4) << sets_log2; }

// The predicate a call's flags ask for; a cache serves the calls whose
// predicate is its own.
STL_SC_HD uint32_t sigcache_predicate(uint32_t flags) { return flags & kScPredicateMask; }

STL_SC_HD uint64_t sigcache_mix(uint64_t h) {
  h ^= h >> 32;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 29;
  return h;
}

// 64-bit hash of the eight ID words under `seed` (every word and the whole
// seed reach every bit of the result), as acctdir_hash.
STL_SC_HD uint64_t sigcache_hash(const uint32_t id[kScIdWords], uint64_t seed) {
  uint64_t h = sigcache_mix(seed + 0x9e3779b97f4a7c15ull);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    h = sigcache_mix((h ^ (id[2 * i] | ((uint64_t)id[2 * i + 1] << 32))) * 0xc4ceb9fe1a85ec53ull);
  h = sigcache_mix((h ^ (8ull << 32)) * 0xc4ceb9fe1a85ec53ull);
  h = sigcache_mix(h + seed * 0xd6e8feb86659fd93ull);
  return h;
}

STL_SC_HD uint32_t sigcache_set(uint64_t hash, uint32_t mask) { return (uint32_t)(hash >> 32) & mask; }
STL_SC_HD uint32_t sigcache_first_way(uint64_t hash) { return (uint32_t)(hash >> 62); }

// An ID that is never stored and never hits: its first 64 bits are zero (the
// all-zero ID among them).
STL_SC_HD bool sigcache_unstorable(const uint32_t id[kScIdWords]) { return (id[0] | id[1]) == 0u; }

// The line of a set as eight 16-byte loads (lines is 128-byte aligned).
STL_SC_HD void sigcache_load_line(const uint32_t* lines, uint32_t set, uint32_t w[kScLineWords]) {
  const uint4* q = reinterpret_cast<const uint4*>(lines + (size_t)set * kScLineWords);
#pragma unroll
  for (uint32_t i = 0; i < kScLineWords / 4; ++i) {
    const uint4 a = q[i];
    w[4 * i] = a.x, w[4 * i + 1] = a.y, w[4 * i + 2] = a.z, w[4 * i + 3] = a.w;
  }
}

// The way of `line` whose 32 bytes equal id, or kScWays.
STL_SC_HD uint32_t sigcache_match(const uint32_t line[kScLineWords], const uint32_t id[kScIdWords]) {
  uint32_t at = kScWays;
#pragma unroll
  for (int w = (int)kScWays - 1; w >= 0; --w) {
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScIdWords; ++j) diff |= line[kScIdWords * w + j] ^ id[j];
    if (diff == 0) at = (uint32_t)w;
  }
  return at;
}

// True iff some way of the ID's set holds all 32 bytes of id.
STL_SC_HD bool sigcache_probe(const uint32_t* lines, uint32_t mask, uint64_t seed, const uint32_t id[kScIdWords]) {
  uint32_t line[kScLineWords];
  sigcache_load_line(lines, sigcache_set(sigcache_hash(id, seed), mask), line);
  return sigcache_match(line, id) != kScWays && !sigcache_unstorable(id);
}

// The host's compare-and-swap (one thread): *p = want if *p == 0; the old *p.
struct ScCasHost {
  uint64_t operator()(uint32_t* p, uint64_t want) const {
    uint64_t old;
    std::memcpy(&old, p, 8);
    if (old == 0) std::memcpy(p, &want, 8);
    return old;
  }
};

// Stores id (see the top).  cas(p, want): the 64-bit compare-and-swap of 0 ->
// want at the 8-byte aligned p, returning what was there.
template <typename Cas>
STL_SC_HD void sigcache_insert(uint32_t* lines, uint32_t mask, uint64_t seed, const uint32_t id[kScIdWords],
                               const Cas& cas) {
  if (sigcache_unstorable(id)) return;
  const uint64_t h = sigcache_hash(id, seed);
  const uint32_t set = sigcache_set(h, mask), first = sigcache_first_way(h);
  uint32_t line[kScLineWords];
  sigcache_load_line(lines, set, line);
  if (sigcache_match(line, id) != kScWays) return;
  uint32_t* base = lines + (size_t)set * kScLineWords;
  const uint64_t id0 = id[0] | ((uint64_t)id[1] << 32);
  for (uint32_t i = 0; i < kScWays; ++i) {
    uint32_t* way = base + kScIdWords * ((first + i) % kScWays);
    const uint64_t old = cas(way, id0);
    if (old == id0) return;
    if (old == 0) {
#pragma unroll
      for (uint32_t j = 2; j < kScIdWords; ++j) way[j] = id[j];
      return;
    }
  }
  uint32_t* way = base + kScIdWords * first;
#pragma unroll
  for (uint32_t j = 0; j < kScIdWords; ++j) way[j] = id[j];
}

}  // namespace stl
