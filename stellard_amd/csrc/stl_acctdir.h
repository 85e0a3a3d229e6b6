// stl_acctdir.h -- launch interface between stl_api.cpp (host) and
// stl_acctdir.hip (gfx950 device code): the account directory (stl_acctdir_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace stl {

// A directory on the device (stl_acctdir_core.h): slots (mask + 1 of them),
// records (12 words each, 16-byte aligned, room for `capacity`), and two
// words of bookkeeping: meta[0] the number of records, meta[1] the longest
// probe sequence any insert has walked.
struct AcctDirDev {
  uint32_t* slots;
  uint32_t* records;
  uint32_t* meta;
  uint32_t mask;
  uint32_t capacity;
  uint64_t seed;
};

// An upsert is these two launches on one stream, in this order.  staged: m
// records with distinct IDs (acctdir_stage); new_idx: m words of scratch.
//   find   a row whose ID is in the map overwrites that record's RegularKey
//          and flags and notes kAdEmpty; any other row takes the next record
//          index (refused, and noted kAdEmpty, at `capacity`), writes the
//          whole record there and notes the index.  Slots are only read.
//   claim  a row with an index puts it into the first empty slot from its
//          home slot on (compare-and-swap), and the walk's length into
//          meta[1] (max).  Records are not read.
hipError_t launch_acctdir_find(const AcctDirDev& dir, const uint32_t* staged, uint32_t m, uint32_t* new_idx,
                               hipStream_t stream);
hipError_t launch_acctdir_claim(const AcctDirDev& dir, const uint32_t* staged, uint32_t m, const uint32_t* new_idx,
                                hipStream_t stream);

// flags[i] = the flags byte of account_id[20 i ..], or STL_ACCT_NOT_FOUND (not
// in the directory, or ABSENT); regular_key (nullable): its RegularKey, zero
// unless HAS_REGULAR_KEY.  account_id and regular_key 4-byte aligned.
hipError_t launch_acctdir_lookup(const AcctDirDev& dir, const uint8_t* account_id, uint32_t n, uint8_t* flags,
                                 uint8_t* regular_key, hipStream_t stream);

// One lane per serialized transaction (rows as launch_tx_signer takes them):
// signer_id and account (both nullable, 4-byte aligned) as that call writes
// them, authority[i] = STL_AUTH_* (stl_acctdir_core.h acctdir_authority_row).
hipError_t launch_acctdir_authority(const AcctDirDev& dir, const uint8_t* blobs, const uint64_t* off,
                                    const uint32_t* len, uint32_t n, uint8_t* signer_id, uint8_t* account,
                                    uint8_t* authority, hipStream_t stream);

}  // namespace stl
