// hostemu_signer.cpp -- TEST HARNESS ONLY.  Compiles the signer-authority
// device code for the host: the one-block SHA-256 and RIPEMD-160 and Hash160
// of stellard_amd/csrc/stl_hash160.h, and the per-row function of
// tx_signer_kernel (stl_signer_core.h), so that tests/test_signer_host.py can
// check them against OpenSSL's digests and a Python restatement on any
// machine.  Not part of the product library.
#include <cstdint>
#include <cstring>

#include "../../stellard_amd/csrc/stl_signer_core.h"

extern "C" {

void hostemu_sha256_32(const uint8_t m[32], uint8_t out[32]) {
  uint32_t w[8], h[8];
  std::memcpy(w, m, 32);
  stl::sha256_32(w, h);
  std::memcpy(out, h, 32);
}

void hostemu_ripemd160_32(const uint8_t m[32], uint8_t out[20]) {
  uint32_t w[8], h[5];
  std::memcpy(w, m, 32);
  stl::ripemd160_32(w, h);
  std::memcpy(out, h, 20);
}

// out[20 i ..] = Hash160(pk[32 i ..])
void hostemu_hash160_32(const uint8_t* pk, size_t n, uint8_t* out) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[8], h[5];
    std::memcpy(w, pk + 32 * i, 32);
    stl::hash160_32(w, h);
    std::memcpy(out + 20 * i, h, 20);
  }
}

// One row of tx_signer_kernel; reads blob[0, len) only.  Returns the authority.
uint32_t hostemu_signer_row(const uint8_t* blob, uint32_t len, uint8_t signer[20], uint8_t account[20],
                            uint32_t* status) {
  uint32_t sg[5], ac[5];
  const uint32_t auth = stl::tx_signer_row(blob, blob, len, sg, ac, status);
  std::memcpy(signer, sg, 20);
  std::memcpy(account, ac, 20);
  return auth;
}

// The Account payload as tx_blob_parse records it: {offset, length}
void hostemu_signer_account_pos(const uint8_t* blob, uint32_t len, uint32_t out[2]) {
  stl::TxLayout t;
  stl::tx_blob_parse(blob, len, t);
  out[0] = t.acct_off;
  out[1] = t.acct_len;
}

}  // extern "C"
