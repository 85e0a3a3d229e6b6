// stl_acctdir_core.h -- the account directory (stl_acctdir_*): a snapshot of
// the three account-root fields Transactor::checkSig reads, keyed by account
// ID, in a form a kernel can probe; and the decision itself.  Plain C++: the
// kernels of stl_acctdir.hip and the host build of
// tests/native/hostemu_acctdir.cpp compile the same functions.
//
// Reference path (Transactor.cpp:151-180, mHasAuthKey set at :326):
//   signer == Account                          -> lsfDisableMaster ? tefMASTER_DISABLED : tesSUCCESS
//   else hasRegularKey && signer == RegularKey -> tesSUCCESS
//   else hasRegularKey                         -> tefBAD_AUTH
//   else                                       -> temBAD_AUTH_MASTER
// and no account root at all is terNO_ACCOUNT before any of it (:312-320).
//
// Layout.  Records of 12 words (48 bytes: three 16-byte loads), appended in
// the order accounts are first seen and never moved:
//   words 0-4  account ID        words 5-9  RegularKey (zero without one)
//   word 10    STL_ACCT_* flags  word 11    zero
// and a map from account ID to record index: open addressing with linear
// probing over a power-of-two number of uint32 slots, at least four per
// record of capacity, so an empty slot always exists and every probe sequence
// ends (the loops are bounded by the slot count all the same).  A slot holds
// a record index or kAdEmpty; the ID is compared in the record the slot names.
// An account that no longer exists keeps its record, flagged ABSENT.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "stl_signer_core.h"

namespace stl {

constexpr uint32_t kAdEmpty = 0xFFFFFFFFu;  // an empty slot; a probe's "not found"
constexpr uint32_t kAdRecWords = 12;
constexpr uint32_t kAdSlotsPerRecord = 4;

// include/stl.h STL_ACCT_*
constexpr uint32_t kAcctHasRegularKey = 0x1;
constexpr uint32_t kAcctMasterDisabled = 0x2;
constexpr uint32_t kAcctAbsent = 0x4;
constexpr uint32_t kAcctFlagMask = 0x7;
constexpr uint32_t kAcctNotFound = 0xFF;

// include/stl.h STL_AUTH_*
constexpr uint32_t kAuthMaster = 0;
constexpr uint32_t kAuthRegular = 1;
constexpr uint32_t kAuthMasterDisabled = 2;
constexpr uint32_t kAuthBadAuth = 3;
constexpr uint32_t kAuthBadAuthMaster = 4;
constexpr uint32_t kAuthNoAccount = 5;
constexpr uint32_t kAuthUndecided = 6;

#define STL_AD_HD __host__ __device__ inline

// Slots of a directory of `capacity` records: the power of two >= 4 * capacity
// (4 at least).  capacity <= 2^24 (STL_ACCTDIR_MAX_ACCOUNTS): no overflow.
STL_AD_HD uint32_t acctdir_slots(uint32_t capacity) {
  uint32_t s = 4;
  while (s < kAdSlotsPerRecord * capacity) s <<= 1;
  return s;
}

STL_AD_HD uint64_t acctdir_mix(uint64_t h) {
  h ^= h >> 32;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 29;
  return h;
}

// 32-bit hash of the five ID words under `seed` (every word and the whole
// seed reach every bit of the result).
STL_AD_HD uint32_t acctdir_hash(const uint32_t id[5], uint64_t seed) {
  uint64_t h = acctdir_mix(seed + 0x9e3779b97f4a7c15ull);
  h = acctdir_mix((h ^ (id[0] | ((uint64_t)id[1] << 32))) * 0xc4ceb9fe1a85ec53ull);
  h = acctdir_mix((h ^ (id[2] | ((uint64_t)id[3] << 32))) * 0xc4ceb9fe1a85ec53ull);
  h = acctdir_mix((h ^ (id[4] | (5ull << 32))) * 0xc4ceb9fe1a85ec53ull);
  h = acctdir_mix(h + seed * 0xd6e8feb86659fd93ull);
  return (uint32_t)(h >> 32);
}

// The record index of account `id`, or kAdEmpty.  slots: mask + 1 of them.
STL_AD_HD uint32_t acctdir_probe(const uint32_t* slots, uint32_t mask, uint64_t seed, const uint32_t* records,
                                 const uint32_t id[5]) {
  uint32_t at = acctdir_hash(id, seed) & mask;
  for (uint32_t i = 0; i <= mask; ++i, at = (at + 1) & mask) {
    const uint32_t idx = slots[at];
    if (idx == kAdEmpty) return kAdEmpty;
    const uint32_t* r = records + (size_t)idx * kAdRecWords;
    uint32_t diff = 0;
#pragma unroll
    for (int w = 0; w < 5; ++w) diff |= r[w] ^ id[w];
    if (diff == 0) return idx;
  }
  return kAdEmpty;
}

// Record idx as three 16-byte loads (records is 16-byte aligned).
STL_AD_HD void acctdir_load(const uint32_t* records, uint32_t idx, uint32_t w[kAdRecWords]) {
  const uint4* q = reinterpret_cast<const uint4*>(records + (size_t)idx * kAdRecWords);
  const uint4 a = q[0], b = q[1], c = q[2];
  w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
  w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
  w[8] = c.x, w[9] = c.y, w[10] = c.z, w[11] = c.w;
}

// Transactor::checkSig for a signer ID and the Account's directory entry
// (found, flags, regular_key), in the reference's branch order: the master
// branch first, so a master-signed row on a MASTER_DISABLED account is
// MASTER_DISABLED even when RegularKey equals the account's own ID.
// regular_key is not looked at without HAS_REGULAR_KEY.  Both comparisons are
// computed on every row (no data-dependent branch on ID bytes).
STL_AD_HD uint32_t acct_authority(const uint32_t signer[5], const uint32_t account[5], bool found, uint32_t flags,
                                  const uint32_t regular_key[5]) {
  uint32_t dm = 0, dr = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    dm |= signer[i] ^ account[i];
    dr |= signer[i] ^ regular_key[i];
  }
  if (!found || (flags & kAcctAbsent)) return kAuthNoAccount;
  if (dm == 0) return (flags & kAcctMasterDisabled) ? kAuthMasterDisabled : kAuthMaster;
  if (flags & kAcctHasRegularKey) return dr == 0 ? kAuthRegular : kAuthBadAuth;
  return kAuthBadAuthMaster;
}

// One row of acctdir_authority_kernel: tx_signer_row on the blob (signer,
// account and status as it gives them), then, where that decided between
// MASTER and NOT_MASTER (an STL_TX_OK row with a 20-byte Account), the
// directory's verdict on the Account; UNDECIDED on every other row.
template <typename Bytes>
STL_AD_HD uint32_t acctdir_authority_row(const Bytes& bytes, const uint8_t* b, uint32_t len, const uint32_t* slots,
                                         uint32_t mask, uint64_t seed, const uint32_t* records, uint32_t signer[5],
                                         uint32_t account[5], uint32_t* status) {
  const uint32_t master = tx_signer_row(bytes, b, len, signer, account, status);
  if (master == kSignerUndecided) return kAuthUndecided;
  const uint32_t idx = acctdir_probe(slots, mask, seed, records, account);
  uint32_t w[kAdRecWords];
#pragma unroll
  for (uint32_t i = 0; i < kAdRecWords; ++i) w[i] = 0u;
  if (idx != kAdEmpty) acctdir_load(records, idx, w);
  return acct_authority(signer, account, idx != kAdEmpty, w[10], w + 5);
}

// ---- host only: an upsert batch as the kernels take it ----
// Checks the batch (a flags byte with unknown bits, or HAS_REGULAR_KEY
// without a regular_key array: false) and writes one 12-word record per
// distinct account ID, the last occurrence of each, in ID order.  A record's
// RegularKey words are zero without HAS_REGULAR_KEY.
inline bool acctdir_stage(const uint8_t* account_id, const uint8_t* flags, const uint8_t* regular_key, size_t m,
                          std::vector<uint32_t>& staged) {
  for (size_t i = 0; i < m; ++i) {
    if (flags[i] & ~kAcctFlagMask) return false;
    if ((flags[i] & kAcctHasRegularKey) && !regular_key) return false;
  }
  std::vector<uint32_t> order(m);
  for (size_t i = 0; i < m; ++i) order[i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const int c = std::memcmp(account_id + 20 * (size_t)a, account_id + 20 * (size_t)b, 20);
    return c != 0 ? c < 0 : a < b;
  });
  staged.clear();
  staged.reserve(m * kAdRecWords);
  for (size_t j = 0; j < m; ++j) {
    const size_t i = order[j];
    if (j + 1 < m && std::memcmp(account_id + 20 * i, account_id + 20 * (size_t)order[j + 1], 20) == 0) continue;
    uint32_t w[kAdRecWords] = {0};
    std::memcpy(w, account_id + 20 * i, 20);
    if (flags[i] & kAcctHasRegularKey) std::memcpy(w + 5, regular_key + 20 * i, 20);
    w[10] = flags[i];
    staged.insert(staged.end(), w, w + kAdRecWords);
  }
  return true;
}

}  // namespace stl
