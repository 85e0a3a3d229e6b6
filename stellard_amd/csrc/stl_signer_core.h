// stl_signer_core.h -- who signed a serialized transaction: one row of
// tx_signer_kernel (stl_signer.hip), also compiled for the host by
// tests/native/hostemu_signer.cpp.
//
// Reference path: after checkSign, Transactor::checkSig (Transactor.cpp:151-170)
// asks whether the signing key is the one authorised for the account,
//   mSigningPubKey.getAccountID() == mTxnAccountID            (master key)
//   else ... == mTxnAccount->getFieldAccount160(sfRegularKey)  (ledger state)
// with getAccountID() = Hash160(key) (RippleAddress.cpp:361-363).  The first
// comparison needs nothing but the blob, so the device answers it; the second
// stays with the caller.
#pragma once
#include "stl_hash160.h"
#include "stl_txblob.h"

namespace stl {

// include/stl.h STL_SIGNER_*
constexpr uint32_t kSignerNotMaster = 0;
constexpr uint32_t kSignerMaster = 1;
constexpr uint32_t kSignerUndecided = 2;

// One transaction blob.  bytes[i], i < len, is the blob for the canonical-form
// pass; b the same bytes for the word readers (blob_words: never outside
// [b, b + len)).  The status is the one tx_blob_parse_kernel reports.
//   STL_TX_OK row:  signer = Hash160(SigningPubKey); with a 20-byte Account,
//                   account = its bytes and the authority is MASTER or
//                   NOT_MASTER; with any other Account length account = 0 and
//                   the authority is UNDECIDED.
//   any other row:  signer = account = 0, UNDECIDED.
template <typename Bytes>
STL_HD uint32_t tx_signer_row(const Bytes& bytes, const uint8_t* b, uint32_t len, uint32_t signer[5],
                              uint32_t account[5], uint32_t* status) {
  const BlobKind kind = blob_kind_tx();
  TxLayout t;
  tx_blob_parse(bytes, len, t, kind.sig_code, kind.min_len, kind.format);
  if (t.status == kTxOk && t.xs1 != len) t.status = kTxDeferred;  // as tx_blob_parse_kernel
  *status = t.status;
#pragma unroll
  for (int i = 0; i < 5; ++i) signer[i] = account[i] = 0u;
  if (t.status != kTxOk) return kSignerUndecided;
  uint32_t pk[8];
  blob_words(pk, b, t.pk_off, 8, len);
  hash160_32(pk, signer);
  if (t.acct_len != 20u) return kSignerUndecided;
  blob_words(account, b, t.acct_off, 5, len);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) diff |= signer[i] ^ account[i];
  return diff == 0 ? kSignerMaster : kSignerNotMaster;
}

}  // namespace stl
