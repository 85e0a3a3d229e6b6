// stl_signer.h -- launch interface between stl_api.cpp (host) and
// stl_signer.hip (gfx950 device code): account IDs and the master-key match
// (stl_account_id_batch*, stl_tx_blob_signer_batch*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace stl {

// account_id[20 i ..] = Hash160(pk[32 i ..]), i < n.  pk 16-byte aligned,
// account_id 4-byte aligned; exactly 20 n bytes are written.
hipError_t launch_account_id(const uint8_t* pk, uint32_t n, uint8_t* account_id, hipStream_t stream);

// One lane per serialized transaction (rows as launch_tx_blob takes them):
// signer_id[20 i ..], account[20 i ..] (nullable) and authority[i]
// (stl_signer_core.h tx_signer_row).  signer_id and account 4-byte aligned.
hipError_t launch_tx_signer(const uint8_t* blobs, const uint64_t* off, const uint32_t* len, uint32_t n,
                            uint8_t* signer_id, uint8_t* account, uint8_t* authority, hipStream_t stream);

}  // namespace stl
