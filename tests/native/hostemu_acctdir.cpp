// hostemu_acctdir.cpp -- TEST HARNESS ONLY.  Compiles the account directory's
// device code (stellard_amd/csrc/stl_acctdir_core.h) for the host: the hash,
// the probe, the decision function and the per-row function of
// acctdir_authority_kernel as they are, and an upsert that runs the two
// launches of stl_acctdir.hip one after the other, one row at a time: first
// every row's find step, then every new row's claim step.  Not part of the
// product library.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stellard_amd/csrc/stl_acctdir_core.h"

namespace {

struct EmuDir {
  uint32_t capacity = 0, mask = 0, count = 0, longest = 0;
  uint64_t seed = 0;
  uint32_t* slots = nullptr;    // exactly mask + 1 words
  uint32_t* records = nullptr;  // exactly 12 * capacity words, 16-byte aligned
};

uint32_t* alloc16(size_t words) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, words * 4) != 0) return nullptr;
  return static_cast<uint32_t*>(p);
}

}  // namespace

extern "C" {

uint32_t hostemu_acctdir_slots(uint32_t capacity) { return stl::acctdir_slots(capacity); }

uint32_t hostemu_acctdir_hash(const uint8_t id[20], uint64_t seed) {
  uint32_t w[5];
  std::memcpy(w, id, 20);
  return stl::acctdir_hash(w, seed);
}

uint32_t hostemu_acct_authority(const uint8_t signer[20], const uint8_t account[20], int found, uint32_t flags,
                                const uint8_t regular_key[20]) {
  uint32_t s[5], a[5], r[5];
  std::memcpy(s, signer, 20);
  std::memcpy(a, account, 20);
  std::memcpy(r, regular_key, 20);
  return stl::acct_authority(s, a, found != 0, flags, r);
}

void* hostemu_acctdir_create(uint32_t capacity, uint64_t seed) {
  EmuDir* d = new EmuDir();
  d->capacity = capacity;
  d->mask = stl::acctdir_slots(capacity) - 1;
  d->seed = seed;
  d->slots = alloc16((size_t)d->mask + 1);
  d->records = alloc16((size_t)capacity * stl::kAdRecWords);
  std::memset(d->slots, 0xFF, ((size_t)d->mask + 1) * 4);
  std::memset(d->records, 0, (size_t)capacity * stl::kAdRecWords * 4);
  return d;
}

void hostemu_acctdir_destroy(void* h) {
  EmuDir* d = static_cast<EmuDir*>(h);
  if (!d) return;
  std::free(d->slots);
  std::free(d->records);
  delete d;
}

// {capacity, records, slots, longest_probe}
void hostemu_acctdir_info(void* h, uint32_t out[4]) {
  const EmuDir* d = static_cast<const EmuDir*>(h);
  out[0] = d->capacity;
  out[1] = d->count;
  out[2] = d->mask + 1;
  out[3] = d->longest;
}

// stl_acctdir_upsert: 0, -22 (a bad batch) or -12 (it does not fit; nothing changed)
int hostemu_acctdir_upsert(void* h, const uint8_t* account_id, const uint8_t* flags, const uint8_t* regular_key,
                           size_t m) {
  EmuDir* d = static_cast<EmuDir*>(h);
  std::vector<uint32_t> staged;
  if (!stl::acctdir_stage(account_id, flags, regular_key, m, staged)) return -22;
  const size_t rows = staged.size() / stl::kAdRecWords;
  if ((size_t)d->count + rows > d->capacity) return -12;
  std::vector<uint32_t> new_idx(rows, stl::kAdEmpty);
  // launch 1: acctdir_find_kernel
  for (size_t t = 0; t < rows; ++t) {
    const uint32_t* w = staged.data() + t * stl::kAdRecWords;
    const uint32_t idx = stl::acctdir_probe(d->slots, d->mask, d->seed, d->records, w);
    if (idx != stl::kAdEmpty) {
      uint32_t* r = d->records + (size_t)idx * stl::kAdRecWords;
      for (int j = 5; j <= 10; ++j) r[j] = w[j];
    } else {
      const uint32_t u = d->count++;
      if (u < d->capacity) {
        std::memcpy(d->records + (size_t)u * stl::kAdRecWords, w, stl::kAdRecWords * 4);
        new_idx[t] = u;
      }
    }
  }
  // launch 2: acctdir_claim_kernel
  for (size_t t = 0; t < rows; ++t) {
    if (new_idx[t] == stl::kAdEmpty) continue;
    uint32_t at = stl::acctdir_hash(staged.data() + t * stl::kAdRecWords, d->seed) & d->mask;
    for (uint32_t p = 0; p <= d->mask; ++p, at = (at + 1) & d->mask) {
      if (d->slots[at] == stl::kAdEmpty) {
        d->slots[at] = new_idx[t];
        if (p + 1 > d->longest) d->longest = p + 1;
        break;
      }
    }
  }
  return 0;
}

// acctdir_lookup_kernel, row by row; regular_key nullable
void hostemu_acctdir_lookup(void* h, const uint8_t* account_id, size_t n, uint8_t* flags, uint8_t* regular_key) {
  const EmuDir* d = static_cast<const EmuDir*>(h);
  for (size_t i = 0; i < n; ++i) {
    uint32_t id[5], w[stl::kAdRecWords] = {0};
    std::memcpy(id, account_id + 20 * i, 20);
    const uint32_t idx = stl::acctdir_probe(d->slots, d->mask, d->seed, d->records, id);
    if (idx != stl::kAdEmpty) stl::acctdir_load(d->records, idx, w);
    const bool there = idx != stl::kAdEmpty && (w[10] & stl::kAcctAbsent) == 0;
    const bool has_key = there && (w[10] & stl::kAcctHasRegularKey) != 0;
    flags[i] = (uint8_t)(there ? w[10] : stl::kAcctNotFound);
    if (regular_key) {
      if (has_key)
        std::memcpy(regular_key + 20 * i, w + 5, 20);
      else
        std::memset(regular_key + 20 * i, 0, 20);
    }
  }
}

// One row of acctdir_authority_kernel; reads blob[0, len) only.
uint32_t hostemu_acctdir_authority_row(void* h, const uint8_t* blob, uint32_t len, uint8_t signer[20],
                                       uint8_t account[20], uint32_t* status) {
  const EmuDir* d = static_cast<const EmuDir*>(h);
  uint32_t sg[5], ac[5];
  const uint32_t auth =
      stl::acctdir_authority_row(blob, blob, len, d->slots, d->mask, d->seed, d->records, sg, ac, status);
  std::memcpy(signer, sg, 20);
  std::memcpy(account, ac, 20);
  return auth;
}

}  // extern "C"
