/*
 * stl.h -- C ABI of libstl, the MI355X (gfx950) batched Ed25519
 * transaction-signature verifier for stellard.
 *
 * Drop-in boundary (reference = hfeeki/stellard, libsodium not vendored):
 *
 *   lower boundary replaced: libsodium
 *     int crypto_sign_verify_detached(const unsigned char *sig,
 *                                     const unsigned char *m,
 *                                     unsigned long long mlen,
 *                                     const unsigned char *pk);
 *     called at src/ripple_data/protocol/RippleAddress.cpp:196-197 and
 *     src/ripple_data/crypto/StellarPublicKey.cpp:73-74
 *   upper boundary mirrored:
 *     bool RippleAddress::verifySignature(uint256 const&, Blob const&) const
 *       src/ripple_data/protocol/RippleAddress.cpp:190-200 (= verify && S<L)
 *     bool SerializedTransaction::checkSign(const RippleAddress&) const
 *       src/ripple_app/misc/SerializedTransaction.cpp:220-230
 *       (= SHA512Half(signing preimage) then verifySignature)
 *
 * Conventions: plain pointers and sizes, caller-owned host buffers, no
 * exceptions across the ABI, nothing retained after return.  Accept bitmaps
 * are ceil(n/8) bytes, bit i = byte i>>3, bit (i & 7), LSB first; a set bit
 * means ACCEPT under stellard's composite predicate (verify && S < L).
 *
 * Return codes: STL_OK (0) or a negative error.  On error the bitmap is
 * undefined and the caller MUST fall back to its own per-signature check --
 * a device error is never reported as a reject.  libstl itself has no CPU
 * verify path.
 */
#ifndef STL_H
#define STL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STL_ABI_VERSION 4

/* ---- return codes ---- */
#define STL_OK 0
#define STL_EINVAL (-22)   /* bad argument (null pointer with n > 0, bad flags, bad length) */
#define STL_ENODEV (-19)   /* no gfx950 device available / not initialised */
#define STL_ENOMEM (-12)   /* device or host allocation failed */
#define STL_EHIP (-1000)   /* HIP runtime error (kernel launch, copy, sync) */
#define STL_ERCCL (-1001)  /* RCCL missing, communicator setup or a collective failed */

/* ---- flags ---- */
/* Accept predicate of crypto_sign_verify_detached to reproduce.  Default is
 * the container's executable oracle, libsodium 1.0.18 (S < L, R and A not of
 * small order, A canonical).  STELLARD_1_0_0 reproduces the ref10-era
 * predicate of the libsodium the reference pins (Dockerfile:9-10): only
 * (sig[63] & 0xE0) == 0, plus a reject of the all-zero key (as some 1.0.x
 * releases did).  Parity for it is unpinned offline; where
 * the offline restatement cannot be pinned the policy errs toward reject,
 * which is the safe side -- the caller re-checks every reject serially. */
#define STL_POLICY_SODIUM_1_0_18 0x0u
#define STL_POLICY_STELLARD_1_0_0 0x1u
#define STL_POLICY_MASK 0x1u
/* stellard's crypto_sign_check_S_lt_l (RippleAddress.cpp:226-252) is always
 * applied (composite predicate); the flag exists for ABI symmetry. */
#define STL_REQUIRE_S_LT_L 0x2u
/* Check every signature with full-length scalars ([S]B - [k]A, 253-bit
 * chain) instead of the half-size-scalar equation.
 * Same accept bits, about 1.6x slower; a cross-check / reference mode. */
#define STL_FULL_LENGTH 0x4u
/* Decode each distinct public key of a batch once (stellard's signers repeat:
 * the configs-1/5 shape is 1,000 accounts for 100k transactions).  Same
 * accept bits; costs a hash pass and extra device workspace: about 270 MB
 * (stl_kernels.h kDedupBytes: hash slots, key arrays, decoded keys, shared and
 * wide key tables), allocated once per device for the host batch API and once
 * per (device, stream) -- per library stream too, and for at most
 * STL_TUNE_STREAM_WORKSPACES caller streams -- for the device-resident API.
 * Does not pay when keys are all distinct.  Chunks small enough for lane
 * pairs or quads (STL_ONE_LANE below) run on them instead: latency-bound
 * there, the pairs and quads are faster. */
#define STL_DEDUP_KEYS 0x8u
/* The host batch calls (stl_ed25519_verify_batch, stl_tx_verify_batch, the
 * blob calls) choose STL_DEDUP_KEYS by themselves for every 64K-row chunk in
 * which a host-side sample of 1,024 evenly spaced keys shows at least a fifth
 * repeating an earlier one (about 40 us per chunk, overlapped with the earlier
 * chunks' kernels); this flag turns the automatic choice off (A/B and callers
 * that know their keys are distinct).  The device-resident verify and
 * checkSign calls choose by feedback instead (their keys are in HBM): each
 * call ends with a one-workgroup sample of 2,048 keys on the caller's stream
 * (dedup when at least a quarter repeat), and the next call on that stream
 * follows that sample's verdict (no synchronisation; a stream's first call
 * runs without dedup).  The bits never depend on the choice. */
#define STL_NO_AUTO_DEDUP 0x20u
/* Small chunks run each signature on two lanes, which ends a launch that
 * cannot fill the device sooner: the main kernel up to
 * a quarter of the device's resident lanes (one pair wave per SIMD; 32,768
 * signatures on 256 CUs), on eight lanes (two lane quads) up to one quad wave
 * per SIMD (8,192 signatures) and on four (two duos) up to one duo wave per
 * SIMD (16,384; STL_TUNE_QUAD), the point decoding on pairs up to half of
 * them.  Same accept bits; this flag turns both off (A/B and
 * tests). */
#define STL_ONE_LANE 0x10u
/* TEST-ONLY: the raw crypto_sign_verify_detached predicate of the selected
 * policy, without stellard's S < L -- what RippleAddress_test expects of the
 * bare libsodium call (RippleAddress.cpp:838-845: under the 1.0.0 policy a
 * signature with S + L verifies).  stellard's accept is always the composite;
 * never set this outside tests. */
#define STL_DEBUG_RAW_PREDICATE 0x80000000u

/* stl_config.flags.  By default every device of a host batch call copies its
 * slice of the accept bitmap to the host.  With STL_CFG_RCCL_GATHER the slices
 * are gathered on device 0 with RCCL over xGMI (ncclGather / grouped
 * send-recv into one buffer, any device count) and copied to the host once;
 * stl_init returns STL_ERCCL if that communicator cannot be built.  (Opt-in
 * until a multi-GPU run has compared the gathered bitmaps: the one-process-
 * per-GPU gather, stl_bitmap_gather_device, is the measured path.) */
#define STL_CFG_RCCL_GATHER 0x1u /* gather the bitmap over RCCL (in-process communicator) */
#define STL_CFG_NO_RCCL 0x2u     /* never use RCCL: every device copies its slice to the host */

/* The caller's own single-signature check, libsodium's signature:
 * stellard passes crypto_sign_verify_detached (libstl never links it). */
typedef int (*stl_verify_fn)(const unsigned char *sig, const unsigned char *m, unsigned long long mlen,
                             const unsigned char *pk);

typedef struct stl_config {
  uint32_t struct_size;       /* sizeof(stl_config); the 16-byte ABI-1 and 24-byte ABI-2 structs
                                 are accepted too */
  int32_t device_count;       /* devices to use; <= 0 = all visible */
  int32_t first_device;       /* first HIP ordinal to use */
  uint32_t flags;             /* STL_CFG_* */
  int32_t shards_per_device;  /* ABI 2: host batch shards per device, each on its own host
                                 thread (<= 0 = 1; more than 1 forces the per-device copy) */
  uint32_t reserved;          /* 0 */
  stl_verify_fn fallback_verify; /* ABI 3, may be NULL: with it, stl_ed25519_verify_detached
                                    answers a device failure (ENODEV, ENOMEM, EHIP, ERCCL)
                                    with fallback_verify(...) == 0 && S < L, so it returns
                                    only 0 or -1 -- libsodium's convention.  Registered even
                                    when stl_init itself then fails for want of a device. */
} stl_config;

/* Replaces/augments sodium_init() (src/ripple_app/ripple_app.cpp:129-132).
 * Idempotent; cfg may be NULL (all devices).  Thread-safe.  When libstl is
 * already running (an earlier stl_init, or the implicit one of a first entry-
 * point call) a cfg still registers its fallback_verify and returns STL_OK if
 * it asks for the live device set, gather mode and shard count, STL_EINVAL
 * otherwise (stl_shutdown first to change them).  Environment
 * overrides: STL_DEVICES (device count), STL_SHARDS_PER_DEVICE, STL_RCCL
 * (1 = as STL_CFG_RCCL_GATHER, 0 = as STL_CFG_NO_RCCL), STL_FAULT_AFTER
 * (stl_debug_fault_after). */
int stl_init(const stl_config *cfg);
void stl_shutdown(void);
int stl_device_count(void);
const char *stl_version(void);
const char *stl_strerror(int rc);

/* Same signature as libsodium's crypto_sign_verify_detached (0 = accept,
 * -1 = reject), plus stellard's S<L: i.e. exactly
 * RippleAddress::verifySignature's bool as 0/-1.  Runs on the GPU (batch of
 * one).  A device failure returns a value < -1 -- unless stl_config's
 * fallback_verify was registered, in which case the call answers with it and
 * only ever returns 0 or -1.  Only with a fallback registered is this a
 * literal drop-in for `crypto_sign_verify_detached(...) == 0` at
 * RippleAddress.cpp:196-197: without one a device error must be told apart
 * from a reject by the caller (rc < -1).  STL_EINVAL (a NULL pointer) is
 * returned either way; a message longer than 2^32 - 1 bytes is STL_EINVAL
 * without a fallback and the fallback's answer (&& S < L) with one.
 * LATENCY: a signature's chain runs on eight GPU lanes (two lane quads), so a
 * call is latency-bound: 295 us per call on MI355X against libsodium's 31 us
 * (round 4; 489 us on lane pairs in round 2), and concurrent calls
 * serialise on the device (tools/latency.py).
 * Callers that verify one signature at a time (stellard's JobQueue workers)
 * keep libsodium, or submit through stl_batcher_* when many requests are in
 * flight; this entry point is the drop-in for correctness, not for speed. */
int stl_ed25519_verify_detached(const uint8_t *sig, const uint8_t *m, unsigned long long mlen,
                                const uint8_t *pk);

/* n signatures over 32-byte messages (the stellard signing hash).
 * sig: n*64 bytes (R || S), msg: n*32, pk: n*32 -- caller host memory.
 * Sharded by index over the initialised devices (contiguous, 64-aligned). */
int stl_ed25519_verify_batch(const uint8_t *sig, const uint8_t *msg, const uint8_t *pk, size_t n,
                             uint8_t *accept_bitmap, uint32_t flags);

/* checkSign equivalent: msg_i = SHA512Half(preimage_i), then verify.
 * preimage_i = preimages[offset[i] .. offset[i]+len[i]) and already includes
 * the 4-byte "STX\0" prefix (HashPrefix::txSign, HashPrefix.cpp:30).  Any
 * prefixed preimage works the same way, e.g. a consensus proposal's 76-byte
 * "PRP\0" || seq || closeTime || prevLedger || position
 * (LedgerProposal::getSigningHash, LedgerProposal.cpp:54-65).  Offsets may
 * come in any order; with several devices the rows are split into
 * contiguous 64-aligned shards of about equal preimage bytes. */
int stl_tx_verify_batch(const uint8_t *preimages, const uint64_t *offset, const uint32_t *len,
                        const uint8_t *sig, const uint8_t *pk, size_t n, uint8_t *accept_bitmap,
                        uint32_t flags);

/* ---- device-resident entry points (asynchronous on the caller's stream) ----
 * All pointers are device pointers on the current HIP device; stream is a
 * hipStream_t (NULL = default stream).  The bitmap is written as
 * ceil(n/64) little-endian 64-bit words (same bit order as above). */
int stl_ed25519_verify_batch_device(const uint8_t *d_sig, const uint8_t *d_msg, const uint8_t *d_pk,
                                    size_t n, uint64_t *d_bitmap_words, uint32_t flags, void *stream);

/* SHA512Half over n preimages -> d_msg (n*32 bytes). */
int stl_tx_hash_batch_device(const uint8_t *d_preimages, const uint64_t *d_offset, const uint32_t *d_len,
                             size_t n, uint8_t *d_msg, void *stream);

/* Device-resident checkSign: SHA512Half(preimage_i) then verify, over rows in
 * HBM (preimages as stl_tx_verify_batch's; d_sig n*64, d_pk n*32).  Cut into
 * the verify's chunks and spread over the caller's stream and one of libstl's,
 * each chunk's hashing right before its verify, so the hashing overlaps the
 * other stream's kernels.  Bits = stl_tx_hash_batch_device followed by
 * stl_ed25519_verify_batch_device on the same stream. */
int stl_tx_verify_batch_device(const uint8_t *d_preimages, const uint64_t *d_offset, const uint32_t *d_len,
                               const uint8_t *d_sig, const uint8_t *d_pk, size_t n, uint64_t *d_bitmap_words,
                               uint32_t flags, void *stream);

/* ---- serialized transactions ----
 * checkSign straight from serialized transactions -- the bytes of
 * TMTransaction.rawTransaction, or what STObject::add writes: n blobs at
 * blobs[offset[i] .. offset[i]+len[i]), each the full transaction including
 * its TxnSignature field.  Replaces, per transaction, the
 * SerializedTransaction(SerializerIterator&) -> getSigningHash ->
 * checkSign sequence (SerializedTransaction.cpp:65-92,162-165,192-230) and
 * getTransactionID (SerializedTransaction.cpp:167-171).  The device splices
 * the signing preimage out of the blob ("STX\0" || blob minus TxnSignature,
 * Signature, TxnSignatures), which equals the reference's re-serialisation
 * when the blob is in canonical form; it checks that form and DEFERS every
 * blob it cannot prove canonical (stellard_amd/csrc/stl_txblob.h lists the
 * rules).  It also restates the constructor's template checks
 * (SerializedTransaction.cpp:79-91: TransactionType present with a TxFormats
 * template, required fields present, no field outside the template), so
 * STL_TX_OK implies the reference constructs the transaction; raw wire bytes
 * are a safe input.  Validations (STL_BLOB_VALIDATION) with a field outside
 * SerializedValidation's template are deferred (the reference drops such a
 * field from the signing hash).  Per-transaction status: */
#define STL_TX_OK 0        /* accept bit = checkSign(); tx_id valid */
#define STL_TX_DEFERRED 1  /* accept bit 0; caller runs its own checkSign; tx_id zero */
#define STL_TX_MALFORMED 2 /* SigningPubKey not 32 B or TxnSignature not 64 B: checkSign()
                              is false (RippleAddress.cpp:192-194); accept bit 0; tx_id valid */

/* status: n bytes or NULL; tx_id: n*32 bytes (SHA512Half("TXN\0" || blob)) or NULL. */
int stl_tx_blob_verify_batch(const uint8_t *blobs, const uint64_t *offset, const uint32_t *len, size_t n,
                             uint8_t *accept_bitmap, uint8_t *status, uint8_t *tx_id, uint32_t flags);

/* The same over other signed STObjects.  kind:
 *   STL_BLOB_TRANSACTION  as stl_tx_blob_verify_batch ("STX\0", TxnSignature;
 *                         id = SHA512Half("TXN\0" || blob))
 *   STL_BLOB_VALIDATION   SerializedValidation::isValid(getSigningHash()):
 *                         SHA512Half("VAL\0" || blob minus Signature) checked
 *                         against SigningPubKey / Signature
 *                         (SerializedValidation.cpp:70-73,96-110,
 *                         HashPrefix.cpp:31); id = SHA512Half(blob), the
 *                         suppression key of PeerImp::recvValidation
 *                         (PeerImp.cpp:1148-1155); blobs shorter than 50 bytes
 *                         (PeerImp.cpp:1134) are deferred. */
#define STL_BLOB_TRANSACTION 0u
#define STL_BLOB_VALIDATION 1u
int stl_signed_blob_verify_batch(uint32_t kind, const uint8_t *blobs, const uint64_t *offset, const uint32_t *len,
                                 size_t n, uint8_t *accept_bitmap, uint8_t *status, uint8_t *id, uint32_t flags);

/* Device-resident first half: writes the verify inputs (d_msg n*32, d_sig
 * n*64, d_pk n*32; a deferred or malformed transaction gets a signature that
 * always rejects), d_status (n bytes) and, if d_tx_id is not NULL, the
 * transaction IDs (n*32).  Follow with stl_ed25519_verify_batch_device on the
 * same stream. */
int stl_tx_blob_prepare_device(const uint8_t *d_blobs, const uint64_t *d_offset, const uint32_t *d_len,
                               size_t n, uint8_t *d_msg, uint8_t *d_sig, uint8_t *d_pk, uint8_t *d_tx_id,
                               uint8_t *d_status, void *stream);
int stl_signed_blob_prepare_device(uint32_t kind, const uint8_t *d_blobs, const uint64_t *d_offset,
                                   const uint32_t *d_len, size_t n, uint8_t *d_msg, uint8_t *d_sig, uint8_t *d_pk,
                                   uint8_t *d_id, uint8_t *d_status, void *stream);
/* The whole device-resident check from serialized objects in one call: the
 * blob pass and the verify chunk by chunk over two streams (as
 * stl_tx_verify_batch_device); d_status (n bytes) required, d_id (n*32) may be
 * NULL.  Bits and status = stl_signed_blob_prepare_device followed by
 * stl_ed25519_verify_batch_device. */
int stl_signed_blob_verify_batch_device(uint32_t kind, const uint8_t *d_blobs, const uint64_t *d_offset,
                                        const uint32_t *d_len, size_t n, uint64_t *d_bitmap_words, uint8_t *d_status,
                                        uint8_t *d_id, uint32_t flags, void *stream);

/* ---- signer authority: account IDs and the master-key match ----
 * After checkSign, Transactor::checkSig (Transactor.cpp:151-170) asks whether
 * the signing key is the key authorised for the account: first
 * mSigningPubKey.getAccountID() == mTxnAccountID (the master key), else the
 * account's RegularKey from ledger state.  getAccountID() of an account public
 * key is Hash160(key) = RIPEMD160(SHA256(key)) (RippleAddress.cpp:361-363,
 * HashUtilities.cpp:22-29).  These calls compute the IDs and the first
 * comparison for a whole batch from the blobs alone; the RegularKey comparison
 * needs ledger state, which the account directory below (stl_acctdir_*) keeps
 * on the device: its stl_acctdir_tx_blob_authority* gives checkSig's whole
 * verdict per row.  Single device; the host forms upload, run the device form
 * and copy back.  A failure is a negative code, never a verdict. */
#define STL_ACCOUNT_ID_BYTES 20u
/* Hash160 of n 32-byte account public keys = RippleAddress::getAccountID
 * (RippleAddress.cpp:361-363).  account_id: n*20 bytes, the digest bytes in
 * OpenSSL's order.  Device form: d_pk 16-byte aligned, d_account_id 4-byte
 * aligned (else STL_EINVAL); exactly n*20 bytes are written. */
int stl_account_id_batch(const uint8_t *pk, size_t n, uint8_t *account_id); /* host memory, synchronous */
int stl_account_id_batch_device(const uint8_t *d_pk, size_t n, uint8_t *d_account_id, void *stream);

#define STL_SIGNER_NOT_MASTER 0u /* Hash160(SigningPubKey) != Account: RegularKey decides (ledger state: stl_acctdir_*) */
#define STL_SIGNER_MASTER 1u     /* == Account: Transactor::checkSig's first branch */
#define STL_SIGNER_UNDECIDED 2u  /* row is not STL_TX_OK, or Account is not 20 bytes: the caller's own path */
/* Serialized transactions as stl_tx_blob_verify_batch takes them.  d_signer_id: n*20; d_account: n*20 or NULL;
 * d_authority: n bytes.  Independent of the verify: says who signed, not whether the signature is good.
 * A row's status is the one stl_tx_blob_prepare_device reports.  STL_TX_OK row: signer_id =
 * Hash160(SigningPubKey); account = the Account field's bytes when it has 20 (else zero, and the row is
 * UNDECIDED).  Any other row: zero IDs, UNDECIDED.  d_signer_id and d_account 4-byte aligned (else
 * STL_EINVAL).  account is also the source account of CanonicalTXSet's apply order (CanonicalTXSet.cpp:75-81). */
int stl_tx_blob_signer_batch_device(const uint8_t *d_blobs, const uint64_t *d_offset, const uint32_t *d_len, size_t n,
                                    uint8_t *d_signer_id, uint8_t *d_account, uint8_t *d_authority, void *stream);
int stl_tx_blob_signer_batch(const uint8_t *blobs, const uint64_t *offset, const uint32_t *len, size_t n,
                             uint8_t *signer_id, uint8_t *account, uint8_t *authority);

/* ---- multi-GPU: one process per GPU ----
 * Verification shards by index with no exchange; the accept bitmaps are
 * gathered with RCCL over xGMI.  rank r owns signatures
 * [r*w*64, (r+1)*w*64) of the whole batch, w = words_per_rank (see
 * stl_shard_range).  Setup: rank 0 calls stl_comm_unique_id and hands the
 * 128 bytes to every rank out of band (stellard: its own config; the bench:
 * torch.distributed over TCP); then every rank calls stl_comm_init_rank on its
 * initialised device, which blocks until all ranks have joined -- or until the
 * RCCL deadline (STL_RCCL_TIMEOUT_S at stl_init, default 120 s, or
 * STL_TUNE_RCCL_TIMEOUT_MS) passes: the communicator is then built
 * nonblocking (ncclCommInitRankConfig, blocking = 0) and polled
 * (ncclCommGetAsyncError); on the deadline it is aborted and the call returns
 * STL_ERCCL, and a later stl_comm_init_rank may try again. */
int stl_comm_unique_id(uint8_t id[128]);
int stl_comm_init_rank(int nranks, int rank, const uint8_t id[128]);
void stl_comm_destroy(void);
/* Aborts the communicator (ncclCommAbort: outstanding collectives end without
 * waiting for peers) -- the teardown after a failed or timed-out gather. */
void stl_comm_abort(void);
/* hipStreamSynchronize(stream) with the RCCL deadline (timeout_ms, or the
 * library's when <= 0) on the gather: the work queued on the stream ahead of
 * the last stl_bitmap_gather(v)_device is waited for first (a lapse of 10x the
 * deadline, or of the library's deadline if longer, there is STL_EHIP and
 * keeps the communicator), then, while the
 * stream has not drained, the communicator's asynchronous error is polled; an
 * RCCL error or the deadline aborts the communicator (which ends a stalled
 * gather's kernels) and returns STL_ERCCL, so a rank whose peers never arrive
 * can fall back instead of hanging.  A gather whose enqueue fails or times
 * out aborts the communicator the same way. */
int stl_comm_sync(void *stream, int timeout_ms);
/* What RCCL itself reports for the communicator libstl gathers over
 * (ncclCommCount / ncclCommUserRank): the one-process-per-GPU communicator of
 * stl_comm_init_rank if there is one, else the in-process communicator of
 * stl_init (the rank of the calling thread's current device).  STL_ERCCL when
 * there is neither. */
int stl_comm_info(int *nranks, int *rank);
/* root >= 0: ncclGather of every rank's d_words (words_per_rank u64 words)
 * into d_all_words on rank root (nranks*words_per_rank words, rank order;
 * other ranks may pass NULL); root < 0: ncclAllGather (every rank receives).
 * Asynchronous on stream. */
int stl_bitmap_gather_device(const uint64_t *d_words, size_t words_per_rank, uint64_t *d_all_words, int root,
                             void *stream);

/* Variable-size gather (byte-balanced shards: config 5's ledger split by
 * preimage bytes, stl_shard_range_bytes; or any unequal index shards): rank r
 * holds d_words = word_offsets[r+1] - word_offsets[r] (= nwords) u64 words,
 * which land at word word_offsets[r] of d_all_words on rank root.
 * word_offsets: nranks+1 host entries, identical on every rank.  Grouped
 * ncclSend / ncclRecv (the root's own slice is a device copy); asynchronous
 * on stream.  STL_EINVAL if nwords disagrees with the offsets.  The argument
 * checks are local to each rank and run before the group is posted: a rank
 * that gets STL_EINVAL (its nwords, or a NULL d_all_words on the root) does
 * not join, and its peers then block in their send / recv -- every rank must
 * pass the same word_offsets and its own slice's size. */
int stl_bitmap_gatherv_device(const uint64_t *d_words, size_t nwords, uint64_t *d_all_words,
                              const uint64_t *word_offsets, int root, void *stream);

/* Shard of [0, n) that rank r of g owns: contiguous, whole 64-signature
 * bitmap words (the layout stl_bitmap_gather_device assumes and the host
 * batch calls use across devices). */
void stl_shard_range(size_t n, int r, int g, size_t *lo, size_t *hi);
/* Byte-balanced shard for variable-length rows (config 5: preimages or blobs
 * of 100 B - 4 KB): boundaries at the 64-aligned row where the prefix sum of
 * len crosses r/g of the total -- each then moved to the nearest multiple of
 * the verify step (one main-kernel wave per SIMD of the first device: 65,536
 * rows on 256 CUs; 65,536 before stl_init) when that moves its byte prefix by
 * at most 2.5 % of one rank's share: the device-resident verify's time rises
 * in steps of that many rows, so a shard just past a step would pay a whole
 * extra step (config 5's 2^20 rows over 2, 4, 8 ranks: exactly 2^20 / g each). */
void stl_shard_range_bytes(const uint32_t *len, size_t n, int r, int g, size_t *lo, size_t *hi);

/* ---- request aggregator ----
 * stellard checks transactions one at a time on JobQueue workers
 * (jtTRANSACTION: PeerImp.cpp:64-73, NetworkOPs.cpp:298-320) and has an unused
 * batching hook, TxQueue::addEntryForSigCheck (TxQueue.h:32-33).  An
 * aggregator takes single requests from any thread and runs them as device
 * batches: a batch starts when max_batch requests are pending or the oldest
 * has waited max_delay_us.  Each request completes through its callback, on
 * the aggregator's worker thread, with one verdict: */
#define STL_VERDICT_REJECT 0
#define STL_VERDICT_ACCEPT 1
#define STL_VERDICT_DEFER 2 /* serialized tx not decided on the device (STL_TX_DEFERRED) */
/* or a negative STL_E* code: the batch failed, run your own check. */
typedef void (*stl_verdict_fn)(void *ctx, int verdict);
typedef struct stl_batcher stl_batcher;

/* flags: policy bits as for the batch calls.  NULL on bad arguments. */
stl_batcher *stl_batcher_create(uint32_t max_batch, uint32_t max_delay_us, uint32_t flags);
/* RippleAddress::verifySignature(hash, sig) for one signature (copied). */
int stl_batcher_submit(stl_batcher *b, const uint8_t *sig, const uint8_t *msg32, const uint8_t *pk,
                       stl_verdict_fn fn, void *ctx);
/* SerializedTransaction::checkSign for one serialized transaction (copied). */
int stl_batcher_submit_tx(stl_batcher *b, const uint8_t *blob, size_t len, stl_verdict_fn fn, void *ctx);
/* Returns when every request submitted before the call has completed.
 * Callbacks run on the aggregator's worker thread and must not call
 * stl_batcher_flush or stl_batcher_destroy on their own aggregator. */
void stl_batcher_flush(stl_batcher *b);
void stl_batcher_stats(stl_batcher *b, uint64_t *submitted, uint64_t *completed, uint64_t *batches);
/* Completes every pending request, then frees the aggregator. */
void stl_batcher_destroy(stl_batcher *b);

/* ---- statistics and tracing (metrics) ----
 * Cumulative since stl_init / stl_reset_stats.  Host side: entry-point calls
 * (the host batch / tx / blob calls), signatures submitted, calls that
 * returned < 0, wall time inside them and in the multi-GPU gather.  Device
 * side (every verify launch, host and device entry points): accept bits
 * written and signatures checked by the full-length fallback path.  Reading
 * the device counters synchronises the devices.  STL_TRACE=1 in the
 * environment at stl_init prints one JSON line per host call on stderr. */
typedef struct stl_stats {
  uint32_t struct_size; /* sizeof(stl_stats) */
  uint32_t reserved;
  uint64_t batches, signatures, errors;
  uint64_t host_ns, gather_ns;
  uint64_t accepted, full_length_lanes;
  /* Phase timing (stl_set_phase_timing(1) or STL_PHASE_TIMING=1; zero when
   * off): summed kernel time of the verify phases, measured with HIP events
   * recorded on the launch stream between the phases of every chunk (at most
   * 2^20 signatures; a timed launch runs its chunks one after another) --
   * [0] phase 1 (the whole of it when it runs as one kernel, the default;
   * SHA-512 + lattice when split, STL_TUNE_FUSED_PREP 0), [1] the point
   * decompression kernel when split and the key-dedup kernels, [2] main
   * (Straus loop), [3] fallback -- and the number of chunks timed. */
  uint64_t phase_ns[4];
  uint64_t phase_chunks;
  /* host batch chunks and device-resident calls that chose STL_DEDUP_KEYS by
   * themselves (STL_NO_AUTO_DEDUP above); a struct without this field
   * (struct_size = its offset) is accepted */
  uint64_t auto_dedup_chunks;
  /* rows whose key's decoding came out of the decoded-key cache (checked
   * against the row's key bytes before use) / rows that decoded their key and
   * offered it to the cache (STL_TUNE_KEY_CACHE below); rows of paths that do
   * not consult the cache count as neither.  A struct without these two
   * fields (struct_size = the offset of the first) is accepted. */
  uint64_t key_cache_hits, key_cache_misses;
} stl_stats;
int stl_get_stats(stl_stats *out);
void stl_reset_stats(void);
/* Enables (on != 0) or disables the phase timing of stl_stats for launches
 * made after the call; returns the previous setting.  Off by default: two
 * event records per phase and chunk. */
int stl_set_phase_timing(int on);

/* ---- testing hooks ----
 * Fault injection: after `calls` further HIP/RCCL calls made by libstl the
 * next one reports failure without running (one shot); calls < 0 disarms.
 * Every entry point then returns < 0 (never a reject bitmap) and the batcher
 * delivers the negative code as the verdict. */
void stl_debug_fault_after(long long calls);
/* Verify with a given k = H(R||A||M) mod L (d_k: n*32 bytes) instead of
 * hashing: drives contrived k (the lattice reduction's full-length fallback)
 * next to ordinary lanes in one wave. */
int stl_debug_verify_k_device(const uint8_t *d_sig, const uint8_t *d_k, const uint8_t *d_pk, size_t n,
                              uint64_t *d_bitmap_words, uint32_t flags, void *stream);
/* Execution tuning, process-wide, for A/B experiments and tests: every setting
 * gives the same accept bits.  Returns the previous value, or STL_EINVAL for
 * an unknown key or a value out of range; value -1 only reads the setting.
 * Takes effect for launches made after the call. */
#define STL_TUNE_FUSED_PREP 0 /* 1 (default): phase 1 (SHA-512, lattice, decodings) as one kernel; 0: two */
#define STL_TUNE_MAIN_QUEUE 1 /* 1 (default): the main kernel's waves pull 64-signature units from a
                                 counter; 0: static grid stride */
#define STL_TUNE_STREAMS 2    /* 1..4: a device-resident verify call runs its chunks on this many
                                 concurrent streams (the caller's plus the library's own, forked
                                 and joined by events; not under stl_set_phase_timing) */
#define STL_TUNE_CHUNK_LOG2 3 /* 15..20: log2 of the signatures per chunk when STL_TUNE_STREAMS > 1;
                                 0 (default): round(n / 2^18) equal chunks, at least two */
#define STL_TUNE_BYTE_SHARDS 4 /* 1: host preimage / blob batches take the byte-balanced shard path even
                                  as one shard (test hook: runs the grouped-gather placement and
                                  rank 0's device copy on one GPU under STL_CFG_RCCL_GATHER) */
#define STL_TUNE_QUAD 5        /* lane groups for the smallest chunks' main kernel, bits: 1 = chunks of
                                  at most one wave per SIMD at eight lanes per signature run on lane
                                  quads (each group formula's four products one per lane), 2 = the
                                  next ones up to one wave per SIMD at four lanes on lane duos (two
                                  products per lane); 3 (default) both, 0 lane pairs only */
#define STL_TUNE_STREAM_WORKSPACES 6 /* 1..64 (default 8, env STL_MAX_STREAM_WORKSPACES): caller streams
                                        per device whose context (verify workspace ~0.44 GB, hash
                                        queue, checkSign scratch) libstl keeps; the least recently
                                        used one beyond it is evicted, its buffers kept as a spare
                                        for the next new caller stream (no device synchronisation) */
#define STL_TUNE_LONG_HASH 8        /* 0..62 (default 8; 0 off): in calls of at most two lane-pair chunks
                                        (65,536 rows on 256 CUs), up to 1,024 of the longest preimages
                                        of more than this many SHA-512 blocks are hashed one per wave
                                        (schedules expanded side by side, rounds reading them from
                                        LDS): the longest row sets a small ledger's hash latency */
#define STL_TUNE_SHARED_KEYS 9       /* 0 / 1 (default 1): with STL_DEDUP_KEYS (or the automatic choice) a
                                        device-resident call of several chunks builds ONE key table for
                                        all of them (the first chunk builds it, the others wait for it),
                                        instead of one per chunk */
#define STL_TUNE_WIDE_MIN_ROWS 10     /* 0..2^20 (default 0): a key table of fewer rows (STL_DEDUP_KEYS or the
                                        automatic choice) builds the 9-entry per-key tables only, never
                                        the wide 137-entry ones (whose build a short call waits for) */
#define STL_TUNE_R_AHEAD 11          /* 0 / 1 (default 1): a one-call checkSign with a shared key table
                                        decodes every row's R on its own stream beside the key table's
                                        build, and the chunks' phase 1 then only combines the two */
#define STL_TUNE_FIRST_CHUNK 12      /* 0..2^20, a multiple of 64 (default 0): a device-resident verify over
                                        several streams starts with a chunk of this many rows (smaller
                                        than the others): the launch's first phase 1 has no main
                                        kernel to overlap */
#define STL_TUNE_RCCL_TIMEOUT_MS 7 /* 1..3,600,000 (default 120,000; env STL_RCCL_TIMEOUT_S): deadline of
                                      stl_comm_init_rank and stl_comm_sync */
#define STL_TUNE_KEY_CACHE 13 /* 0..K (default K; 0 off): log2 of the sets in use of the decoded-key
                                 cache, K being the log2 of the sets each device allocated at stl_init
                                 (env STL_KEY_CACHE_LOG2: 10..24, default 20 = 256 MB per device; 0: no
                                 cache).  Chunks that run one lane per signature without key dedup
                                 look each row's key up in the cache -- 2^K sets of 6 slots {key tag,
                                 x of the decoded -A}, kept from call to call -- and decode only the
                                 keys they do not find, caching them.  A slot's x is used only after
                                 the curve equation and the sign are checked against the row's own key
                                 bytes, so whatever a slot holds the accept bits are those of a fresh
                                 decoding.  A smaller value only masks the set index; entries left
                                 from another value are harmless. */
#define STL_TUNE_SHAMAP_LOOKUP_BUCKETS 14 /* 0 / 1 (default 1): stl_shamap_tree_lookup* bisects the key's
                                             bucket; 0 bisects the whole array (the A/B run of
                                             tools/shamap_lookup_bench.py): the same outputs */
int stl_debug_tuning(int key, int value);
/* Caller-stream contexts libstl currently keeps on the current device. */
int stl_debug_stream_contexts(void);
/* The current device's decoded-key cache.  _clear zeroes it (every slot
 * empty) on the library's stream and waits for that; calls in flight on other
 * streams are not waited for.  _info reports its device address, size in bytes
 * (0: none), log2 of its sets and slots (ways) per set.  Set i is the 256
 * bytes from byte 256 i: way w's 8-byte key tag at byte 8 w, the 32 canonical
 * little-endian bytes of its x(-A) at byte 64 + 32 w (stl_keycache.h).  Tests
 * write into it to show that no content changes an accept bit.  STL_ENODEV
 * before stl_init. */
int stl_debug_key_cache_clear(void);
int stl_debug_key_cache_info(void **d_base, uint64_t *bytes, uint32_t *sets_log2, uint32_t *ways);
/* Measurement only (bench.py clock_ghz): enqueues nwg one-wave workgroups on
 * `stream`; workgroup i writes d_out[4i..4i+3] = {shader cycle counter
 * (s_memtime), 100 MHz counter (s_memrealtime), XCC_ID register, HW_ID
 * register}.  Two stamps around a timed region give its average shader clock
 * per XCD.  STL_EINVAL for a null d_out or nwg > 65,536. */
int stl_debug_clock_stamp(uint64_t *d_out, uint32_t nwg, void *stream);
/* Tests only: the field, scalar and group arithmetic under the verify kernels,
 * one function at a time, as the device compiles it.  _ops runs op (an index
 * into the table of stellard_amd/csrc/stl_selftest.h, which also documents the
 * row formats) on n rows, one lane per row: row i is the STL_SELFTEST_IN_WORDS
 * 32-bit words from d_in + STL_SELFTEST_IN_WORDS * i (raw limbs or scalar
 * words, nothing reduced), its result the STL_SELFTEST_OUT_WORDS words at
 * d_out + STL_SELFTEST_OUT_WORDS * i.  _group runs a lane-group formula of the
 * small-batch kernels on nrows rows, row r on all G lanes of group r (G = 2 or
 * 4); every lane writes its own record, so d_out receives nrows * G records,
 * record G r + j from lane j of group r.  Nothing outside those records is
 * written.  STL_EINVAL for an op outside the table, G other than 2 or 4, more
 * than STL_SELFTEST_MAX_ROWS rows, or a null pointer with rows to run. */
#define STL_SELFTEST_OPS 47
#define STL_SELFTEST_GROUP_OPS 7
#define STL_SELFTEST_IN_WORDS 72
#define STL_SELFTEST_OUT_WORDS 40
#define STL_SELFTEST_MAX_ROWS 1048576
int stl_debug_selftest_ops_device(uint32_t op, const uint32_t *d_in, size_t n, uint32_t *d_out, void *stream);
int stl_debug_selftest_group_device(uint32_t op, uint32_t G, const uint32_t *d_in, size_t nrows, uint32_t *d_out,
                                    void *stream);

/* Drops libstl's context of a caller stream on the current device -- its
 * verify workspace, hash queue, checkSign scratch and events -- without
 * waiting for anything: the buffers join the device's spare list (at most
 * STL_TUNE_STREAM_WORKSPACES sets; stl_shutdown frees them), and the next new
 * caller stream adopts a set, its first kernels ordered on the device behind
 * the last kernels that used it.  Call it before destroying a stream the
 * library has run on, or let the per-device cap evict the least recently
 * used context the same way.  A call still running on that stream keeps the
 * context until it returns.  STL_EINVAL for one of libstl's own pool streams;
 * STL_OK if there is none. */
int stl_release_stream(void *stream);

/* Synthetic-data helpers (RippleAddress::sign, RippleAddress.cpp:254-263;
 * EdKeyPair::setSeed, EdKeyPair.cpp:25-33): RFC 8032 keypair from a 32-byte
 * seed and a detached signature over a 32-byte message. */
int stl_ed25519_sign_batch_device(const uint8_t *d_seed, const uint8_t *d_msg, size_t n, uint8_t *d_pk,
                                  uint8_t *d_sig, void *stream);
/* Test data only: the same rows, then row i with d_cls[i] in 1..11 mutated
 * into SURVEY.md Appendix-B class B<cls> with the 32-bit parameter
 * d_param[i] (the construction of tests/datasets.py, stated in
 * stl_kernels.hip adversarial_row: bit flips, S+L, S >= 2^253, small-order
 * keys and R, mixed-order keys re-signed over A+T, non-canonical and off-curve
 * keys, non-canonical R); d_msg_out receives every row's message (d_cls[i] = 0
 * leaves the row honest). */
int stl_debug_sign_adversarial_device(const uint8_t *d_seed, const uint8_t *d_msg, const uint8_t *d_cls,
                                      const uint32_t *d_param, size_t n, uint8_t *d_pk, uint8_t *d_sig,
                                      uint8_t *d_msg_out, void *stream);

/* ---- registered signer sets (keysets) ----
 * For signers known in advance -- stellard's UNL validators (validations and
 * proposals), a ledger's funded accounts -- libstl keeps, per key, a
 * fixed-window table of j * 2^(8w) * (-A) on the device (and one of B), so a
 * verification is 64 table additions and no doubling:
 * encode([S]B + [k](-A)) == R, the predicate of the per-signature calls bit
 * for bit (the table is built on the decoded point itself, so mixed-order,
 * small-order, non-canonical and undecodable keys answer as they do there
 * under the call's policy).  A row names its signer by its index in the set,
 * or -- the *_by_key calls and stl_keyset_lookup_device -- by its 32-byte
 * public key: the keyset carries a key -> index hash map on the device (first
 * index of a duplicate, as stl_keyset_find; at most 64 KiB, not counted in
 * table_bytes), and a by-key call verifies the rows of registered signers from
 * the tables and every other row with the per-signature kernels, so its bits
 * equal stl_ed25519_verify_batch_device's on every input: the set need not be
 * closed (signers funded after registration, validations from outside the UNL).
 * A keyset lives on one device (the calling thread's current device at
 * creation; the multi-GPU sharding of the host batch calls does not apply) and
 * holds table_bytes of device memory: 512 KiB per key plus the base table. */
#define STL_KEYSET_MAX_KEYS 4096u  /* 2 GiB of tables */
#define STL_KEYSET_BASE 0xFFFFFFFFu /* stl_debug_keyset_rows: the base point's table */
typedef struct stl_keyset stl_keyset;
typedef struct stl_keyset_info {
  uint32_t struct_size; /* sizeof(stl_keyset_info) */
  uint32_t nkeys;
  uint32_t window_bits, windows, rows_per_window, row_bytes; /* table geometry: signed digits of
                                                                window_bits bits, rows |j| = 1..rows_per_window */
  int32_t device;       /* HIP device ordinal */
  uint32_t reserved;
  uint64_t table_bytes; /* device memory of the tables, the base point's included */
} stl_keyset_info;
/* pk: nkeys * 32 bytes, host memory; nkeys in 1..STL_KEYSET_MAX_KEYS; duplicates allowed; flags 0.
 * Synchronous: decodes the keys and builds the tables on the device before returning (the build's
 * scratch is freed again).  STL_OK and *out, or a negative code and *out = NULL. */
int stl_keyset_create(const uint8_t *pk, size_t nkeys, uint32_t flags, stl_keyset **out);
/* Waits for the device work using the keyset, then frees it.  NULL, a destroyed handle and a
 * handle from before stl_shutdown (which frees every keyset) are ignored. */
void stl_keyset_destroy(stl_keyset *ks);
int stl_keyset_get_info(const stl_keyset *ks, stl_keyset_info *out);
/* First index of the 32-byte key in the set, or -1 (also for a handle that is not live); a host-side map. */
long long stl_keyset_find(const stl_keyset *ks, const uint8_t pk[32]);
/* Row i is (key_index[i], sig[64 i..], msg[32 i..]).  flags: the policy bit, STL_REQUIRE_S_LT_L,
 * STL_DEBUG_RAW_PREDICATE; anything else is STL_EINVAL (the execution flags do not apply).  A handle
 * that is not live, or a call on another device than the keyset's, is STL_EINVAL.
 * Host form: host memory, synchronous; a key_index >= nkeys is STL_EINVAL (nothing is verified). */
int stl_keyset_verify_batch(stl_keyset *ks, const uint32_t *key_index, const uint8_t *sig, const uint8_t *msg,
                            size_t n, uint8_t *accept_bitmap, uint32_t flags);
/* Device form: device memory, enqueued on `stream`, bitmap words as stl_ed25519_verify_batch_device
 * writes them.  The indices are not visible to the host here: a row whose key_index >= nkeys gets
 * accept bit 0 (and reads no table); the other rows are unaffected. */
int stl_keyset_verify_batch_device(stl_keyset *ks, const uint32_t *d_key_index, const uint8_t *d_sig,
                                   const uint8_t *d_msg, size_t n, uint64_t *d_bitmap_words, uint32_t flags,
                                   void *stream);
/* checkSign / validation form: SHA512Half of every signing preimage (the kernel of
 * stl_tx_hash_batch_device) into the stream context's scratch, then the keyset verify: the same
 * bits as that call followed by stl_keyset_verify_batch_device. */
int stl_keyset_tx_verify_batch_device(stl_keyset *ks, const uint32_t *d_key_index, const uint8_t *d_preimages,
                                      const uint64_t *d_offset, const uint32_t *d_len, const uint8_t *d_sig,
                                      size_t n, uint64_t *d_bitmap_words, uint32_t flags, void *stream);
/* ---- keysets by public key ----
 * Key index of every row's key: d_key_index[i] = the first index of d_pk[32 i ..] in the set, or
 * STL_KEYSET_NOT_FOUND.  Asynchronous on `stream`; device memory, d_pk 16-byte aligned.
 * d_miss_count (nullable): one uint32 in device memory, set to the number of rows not found.
 * Followed by stl_keyset_verify_batch_device on the same stream this is the fully asynchronous
 * closed-set check: a row of an unregistered signer gets accept bit 0. */
#define STL_KEYSET_NOT_FOUND 0xFFFFFFFFu
int stl_keyset_lookup_device(stl_keyset *ks, const uint8_t *d_pk, size_t n, uint32_t *d_key_index,
                             uint32_t *d_miss_count, void *stream);
/* Open-set verify: row i is (d_pk[32 i..], d_sig[64 i..], d_msg[32 i..]), all 16-byte aligned; the
 * bits of stl_ed25519_verify_batch_device(d_sig, d_msg, d_pk, ...) under the same policy, for every
 * input.  Rows whose key is registered are verified from the tables; the others ("misses") are
 * gathered, verified by the per-signature kernels and their bits put back.  flags as
 * stl_keyset_verify_batch_device.  *misses (nullable): the number of rows of unregistered signers.
 * SYNCHRONISATION: the call waits once on `stream`, for its lookup kernel (an event recorded behind
 * it) -- the host has to learn the miss count before it can size and launch the per-signature
 * kernels.  The keyset verify of all n rows is enqueued before that wait and runs during it;
 * everything else is asynchronous, and the bitmap is complete when `stream` reaches the call's end.
 * The stream context holds the call's buffers: 8 B per row, 128 B per miss. */
int stl_keyset_verify_by_key_device(stl_keyset *ks, const uint8_t *d_pk, const uint8_t *d_sig,
                                    const uint8_t *d_msg, size_t n, uint64_t *d_bitmap_words, uint32_t flags,
                                    void *stream, size_t *misses);
/* Host form: host memory, synchronous (uploads on the device's stream, then the device path). */
int stl_keyset_verify_by_key(stl_keyset *ks, const uint8_t *pk, const uint8_t *sig, const uint8_t *msg, size_t n,
                             uint8_t *accept_bitmap, uint32_t flags);
/* Serialized validations / transactions in device memory (the UNL-validation and ledger-close
 * binding): the pass of stl_signed_blob_prepare_device into the stream context (128 B per row), then
 * the by-key verify on each row's SigningPubKey.  Bits, d_status and d_id (nullable) as
 * stl_signed_blob_verify_batch_device writes them; synchronisation and *misses as
 * stl_keyset_verify_by_key_device. */
int stl_keyset_signed_blob_verify_batch_device(stl_keyset *ks, uint32_t kind, const uint8_t *d_blobs,
                                               const uint64_t *d_offset, const uint32_t *d_len, size_t n,
                                               uint64_t *d_bitmap_words, uint8_t *d_status, uint8_t *d_id,
                                               uint32_t flags, void *stream, size_t *misses);
/* Test hook: nrows table rows from first_row (row = w * rows_per_window + j - 1) of key `key`
 * (STL_KEYSET_BASE: the base point's table) copied to host memory, row_bytes / 4 words each. */
int stl_debug_keyset_rows(const stl_keyset *ks, uint32_t key, uint32_t first_row, uint32_t nrows,
                          uint32_t *out_words);

/* ---- account directory: Transactor::checkSig's verdict per row ----
 * checkSig (Transactor.cpp:151-180, mHasAuthKey set at :326) decides from three fields of the
 * account root:
 *   signer == Account                          -> lsfDisableMaster ? tefMASTER_DISABLED : tesSUCCESS
 *   else hasRegularKey && signer == RegularKey -> tesSUCCESS
 *   else hasRegularKey                         -> tefBAD_AUTH
 *   else                                       -> temBAD_AUTH_MASTER
 * and without an account root the transactor has stopped before (:312-320).  A directory keeps those
 * fields on the device, keyed by account ID and updatable per ledger, so the pass that walks the blob
 * and hashes the signing key (stl_tx_blob_signer_batch_device) gives the final answer: one byte per
 * row, and nothing else need go back to the host.
 * THE ANSWER IS A SNAPSHOT: checkSig against the account state as last upserted.  A SetRegularKey or
 * AccountSet earlier in the same apply order changes the account, so the caller re-decides the rows
 * whose account an earlier transaction of the set touched.
 * Device: a directory lives on one device, the calling thread's current device at creation, like a
 * keyset; a call on another device, or with a handle that is not live, is STL_EINVAL.  It holds
 * `bytes` of device memory: 48 B per account of capacity plus at least 16 B of slots (a hash map at a
 * load of 1/4 at most), and while it has been upserted to, a staging buffer of 52 B per row of the
 * largest batch.
 * Concurrency: the caller must not run stl_acctdir_upsert concurrently with lookups (lookup,
 * tx_blob_authority) on the same directory, work still in flight on a stream included, nor destroy
 * a directory with calls in flight on other threads.  Lookups may run concurrently with each other.
 * A failure is a negative code, never a verdict. */
#define STL_ACCT_HAS_REGULAR_KEY 0x1u   /* sfRegularKey present */
#define STL_ACCT_MASTER_DISABLED 0x2u   /* lsfDisableMaster */
#define STL_ACCT_ABSENT 0x4u            /* upsert: the account root no longer exists */
#define STL_ACCT_NOT_FOUND 0xFFu        /* lookup: not in the directory, or ABSENT */
#define STL_ACCTDIR_MAX_ACCOUNTS 16777216u
#define STL_AUTH_MASTER 0u            /* tesSUCCESS, mSigMaster */
#define STL_AUTH_REGULAR 1u           /* tesSUCCESS by RegularKey */
#define STL_AUTH_MASTER_DISABLED 2u   /* tefMASTER_DISABLED */
#define STL_AUTH_BAD_AUTH 3u          /* tefBAD_AUTH */
#define STL_AUTH_BAD_AUTH_MASTER 4u   /* temBAD_AUTH_MASTER */
#define STL_AUTH_NO_ACCOUNT 5u        /* no such account in the directory (terNO_ACCOUNT is the caller's call) */
#define STL_AUTH_UNDECIDED 6u         /* row not STL_TX_OK, or Account not 20 bytes */
typedef struct stl_acctdir stl_acctdir;
typedef struct stl_acctdir_info {
  uint32_t struct_size;   /* sizeof(stl_acctdir_info) */
  uint32_t capacity;      /* records the directory has room for */
  uint32_t records;       /* records in use: accounts ever upserted (ABSENT ones included), plus any lost
                             to a failed upsert */
  uint32_t slots;         /* of the hash map: the power of two >= 4 * capacity */
  uint32_t longest_probe; /* longest probe sequence an insert has walked */
  int32_t device;         /* HIP device ordinal */
  uint64_t bytes;         /* device memory of slots and records */
  uint64_t seed;          /* of the map's hash */
} stl_acctdir_info;
/* capacity in 1..STL_ACCTDIR_MAX_ACCOUNTS; seed of the map's hash, 0: chosen at random (so account
 * IDs cannot be made to collide).  Synchronous.  STL_OK and *out, or a negative code and *out = NULL. */
int stl_acctdir_create(uint32_t capacity, uint64_t seed, stl_acctdir **out);
/* Waits for the device, then frees the directory.  NULL, a destroyed handle and a handle from before
 * stl_shutdown (which frees every directory) are ignored. */
void stl_acctdir_destroy(stl_acctdir *dir);
int stl_acctdir_get_info(const stl_acctdir *dir, stl_acctdir_info *out);
/* Sets m accounts' state: account_id m*20 bytes, flags m bytes (STL_ACCT_HAS_REGULAR_KEY,
 * STL_ACCT_MASTER_DISABLED, STL_ACCT_ABSENT; any other bit is STL_EINVAL), regular_key m*20 bytes, read
 * only in rows with HAS_REGULAR_KEY (NULL allowed when no row has it, else STL_EINVAL).  Host memory,
 * synchronous.  The batch's IDs are made distinct on the host: the last occurrence of an ID wins.  An
 * account not yet in the directory takes one record, for good: STL_ACCT_ABSENT keeps the record, and
 * later lookups say not found.  When records + distinct IDs of the batch > capacity the call is
 * refused with STL_ENOMEM before any device work (the IDs already present count too: the host does
 * not know them), and the directory is unchanged.
 * A call that fails after it started device work (STL_EHIP, or STL_ENOMEM for its staging buffer) may
 * have applied any part of the batch, and may have used up to m records of capacity; applying the
 * same batch again completes it.  Lookups never see anything but the old or the new state of a whole
 * account. */
int stl_acctdir_upsert(stl_acctdir *dir, const uint8_t *account_id, const uint8_t *flags,
                       const uint8_t *regular_key, size_t m);
/* The device calls: device memory, asynchronous on `stream`.  Before any device work: a NULL
 * required pointer, an ID array (d_account_id, d_regular_key, d_signer_id, d_account) that is not
 * 4-byte aligned, or n > 0xffffffc0 is STL_EINVAL; n == 0 is STL_OK; without a device STL_ENODEV.
 * The bare map: d_flags[i] = the flags byte of d_account_id[20 i ..], or STL_ACCT_NOT_FOUND (never
 * upserted, or ABSENT); d_regular_key (n*20, or NULL): its RegularKey, zero unless HAS_REGULAR_KEY.
 * Exactly n and n*20 bytes are written. */
int stl_acctdir_lookup_device(stl_acctdir *dir, const uint8_t *d_account_id, size_t n, uint8_t *d_flags,
                              uint8_t *d_regular_key, void *stream);
/* Rows, d_signer_id (n*20, or NULL) and d_account (n*20, or NULL) as stl_tx_blob_signer_batch_device
 * takes and writes them, bit for bit.  d_authority[i]: for a row that call decides (STL_TX_OK with a
 * 20-byte Account) the STL_AUTH_* verdict of the branches above on the Account's entry, the master
 * branch first (a master-signed row on a MASTER_DISABLED account is MASTER_DISABLED whatever its
 * RegularKey); STL_AUTH_UNDECIDED for every other row.  One kernel: no workspace, no host wait. */
int stl_acctdir_tx_blob_authority_device(stl_acctdir *dir, const uint8_t *d_blobs, const uint64_t *d_offset,
                                         const uint32_t *d_len, size_t n, uint8_t *d_signer_id,
                                         uint8_t *d_account, uint8_t *d_authority, void *stream);
/* Host form: host memory, synchronous (upload, the device form, copy back); signer_id and account
 * may be NULL. */
int stl_acctdir_tx_blob_authority(stl_acctdir *dir, const uint8_t *blobs, const uint64_t *offset,
                                  const uint32_t *len, size_t n, uint8_t *signer_id, uint8_t *account,
                                  uint8_t *authority);

/* ---- verified-ID cache: rows already accepted skip the Ed25519 verify ----
 * stellard verifies the same transaction several times: on ingest, when a peer's proposed set is
 * acquired, at ledger close and on every retry pass, and for held transactions.  Its answer is
 * HashRouter's SF_SIGGOOD flag, keyed by transaction ID (IHashRouter.h:27-33).  A sigcache is the
 * device-resident counterpart: the IDs of the rows libstl's own verify has accepted, in device
 * memory from one call to the next.  stl_sigcache_signed_blob_verify_batch_device runs the blob pass
 * (parse, both hashes) on every row, probes the cache with each STL_TX_OK row's ID, gives a row that
 * is found accept bit 1 and sends only the others through the per-signature kernels; the rows those
 * accept are inserted.  The ID (SHA512Half("TXN\0" || blob), for a validation SHA512Half(blob))
 * commits to every byte of the blob, and the accept bit is a function of the blob and the predicate
 * alone, so a hit is the verdict: it never goes stale and needs no ledger state.  Only accepts are
 * kept; a rejected, deferred or malformed row is decided anew in every call.
 * CONTRACT: for every input, cache state and interleaving with other calls on the same cache,
 * d_bitmap_words, d_status and d_id are what stl_signed_blob_verify_batch_device writes for the same
 * rows, kind and flags.
 * Binding: a cache is made for one blob kind and one accept predicate,
 * flags & (STL_POLICY_MASK | STL_DEBUG_RAW_PREDICATE).  A verify call with another predicate is
 * STL_EINVAL before any device work; the flags that do not change bits (STL_FULL_LENGTH,
 * STL_DEDUP_KEYS, STL_NO_AUTO_DEDUP, STL_ONE_LANE) are the call's own.
 * Layout: 2^sets_log2 sets of one 128-byte line, 4 ways of a 32-byte ID, 128 << sets_log2 bytes in
 * all; the set comes from a seeded hash of the ID.  A set that receives a fifth ID overwrites one:
 * capacity is the only reason an ID leaves (no expiry), and stl_sigcache_clear the only other.
 * While a set has received at most 4 distinct IDs since creation or clear all of them are present
 * once the inserting work has completed (stl_sigcache_core.h states it exactly).
 * Device: a cache lives on one device, the calling thread's current device at creation, like a
 * keyset; a call on another device, or with a handle that is not live, is STL_EINVAL;
 * stl_shutdown frees every cache.
 * Concurrency: verify calls, lookups and clears on one cache may run concurrently from several
 * threads and streams (a racing insert may or may not survive a clear; how soon one stream's
 * inserts are seen by another only moves the hit rate).  Only destroy needs quiescence.
 * A failure is a negative code, never a verdict; a failed call may leave out inserts, but never
 * inserts an ID whose verify did not run. */
#define STL_SIGCACHE_MAX_SETS_LOG2 24u /* 2 GiB */
#define STL_SIGCACHE_WAYS 4u
typedef struct stl_sigcache stl_sigcache;
typedef struct stl_sigcache_info {
  uint32_t struct_size; /* sizeof(stl_sigcache_info) */
  uint32_t sets_log2;
  uint32_t ways;        /* STL_SIGCACHE_WAYS */
  uint32_t kind;        /* STL_BLOB_* */
  uint32_t predicate;   /* flags & (STL_POLICY_MASK | STL_DEBUG_RAW_PREDICATE) */
  int32_t device;       /* HIP device ordinal */
  uint64_t bytes;       /* device memory of the sets: 128 << sets_log2 */
  uint64_t seed;        /* of the set hash */
} stl_sigcache_info;
/* sets_log2 in 0..STL_SIGCACHE_MAX_SETS_LOG2; kind STL_BLOB_TRANSACTION or STL_BLOB_VALIDATION; flags:
 * the predicate (the policy bit, STL_DEBUG_RAW_PREDICATE; STL_REQUIRE_S_LT_L is accepted), anything
 * else is STL_EINVAL; seed of the set hash, 0: chosen at random (so a peer cannot grind IDs into one
 * set).  Synchronous.  STL_OK and *out, or a negative code and *out = NULL. */
int stl_sigcache_create(uint32_t sets_log2, uint32_t kind, uint32_t flags, uint64_t seed, stl_sigcache **out);
/* Waits for the device, then frees the cache.  NULL, a destroyed handle and a handle from before
 * stl_shutdown are ignored.  No call on the cache may be running on another thread. */
void stl_sigcache_destroy(stl_sigcache *c);
int stl_sigcache_get_info(const stl_sigcache *c, stl_sigcache_info *out);
/* Empties the cache: a memset enqueued on `stream`, asynchronous. */
int stl_sigcache_clear(stl_sigcache *c, void *stream);
/* The bare probe: bit i of d_hit_words = the 32-byte ID d_id[32 i ..] is present.  Device memory,
 * d_id 16-byte aligned, asynchronous on `stream`; ceil(n / 64) words are written whole (the last
 * word's tail bits are zero). */
int stl_sigcache_lookup_device(stl_sigcache *c, const uint8_t *d_id, size_t n, uint64_t *d_hit_words,
                               void *stream);
/* The cached checkSign of serialized objects in device memory; rows, d_bitmap_words, d_status and
 * d_id (nullable, 16-byte aligned) as stl_signed_blob_verify_batch_device takes and writes them, the
 * kind is the cache's.  flags: as that call's, with the cache's predicate.  *hits (nullable): the
 * STL_TX_OK rows found in the cache; *verified (nullable): the STL_TX_OK rows that were not, which
 * went through the per-signature kernels.  With every STL_TX_OK row a hit no per-signature kernel
 * is launched.  Before any device work: a NULL required pointer, n > 0xffffffc0, an unknown flag
 * bit, a misaligned d_id or another predicate than the cache's is STL_EINVAL; n == 0 is STL_OK.
 * SYNCHRONISATION: the call waits once on `stream`, for its probe kernel (an event recorded behind
 * the copy of the miss count) -- the host has to learn the miss count before it can size and launch
 * the per-signature kernels.  Everything else is asynchronous: the gather of the misses, their
 * verify, the scatter of their bits and, last, the insert; the outputs are complete when `stream`
 * reaches the call's end.  The stream context holds the call's buffers: 164 B per row (132 B with
 * d_id given), 128 B per miss. */
int stl_sigcache_signed_blob_verify_batch_device(stl_sigcache *c, const uint8_t *d_blobs, const uint64_t *d_offset,
                                                 const uint32_t *d_len, size_t n, uint64_t *d_bitmap_words,
                                                 uint8_t *d_status, uint8_t *d_id, uint32_t flags, void *stream,
                                                 size_t *hits, size_t *verified);
/* Host form: host memory, synchronous (upload, the device form, copy back); accept_bitmap, status
 * and id (nullable) as stl_signed_blob_verify_batch writes them. */
int stl_sigcache_signed_blob_verify_batch(stl_sigcache *c, const uint8_t *blobs, const uint64_t *offset,
                                          const uint32_t *len, size_t n, uint8_t *accept_bitmap, uint8_t *status,
                                          uint8_t *id, uint32_t flags, size_t *hits, size_t *verified);

/* ---- SHAMap root: the hash that names a set ----
 * Consensus names a transaction set by the root hash of its SHAMap: a proposal's position, the
 * check of an acquired set (LedgerConsensus.cpp:338), a ledger header's txHash, CanonicalTXSet's
 * salt (LedgerConsensus.cpp:969).  The shape of the tree is a function of the set of keys
 * (SHAMap.cpp:680-849: a leaf sits at the shallowest depth where its nibble prefix is unique, under
 * the root at the least), an inner node hashes as SHA512Half("MIN\0" || 16 child hashes, zeros for
 * an empty branch) (SHAMapTreeNode.cpp:257-274), and the empty map's root is 32 zero bytes.  So the
 * root is a function of the keys and their leaf hashes alone.  For a tree without metadata
 * (tnTRANSACTION_NM) the leaf hash is the key, the transaction ID; for the closed ledger's
 * transaction tree and the state tree the leaf hashes come from stl_tx_hash_batch_device over the
 * prefixed leaf preimages.
 *
 * d_key: n * 32 bytes; d_leaf_hash: n * 32 bytes, or NULL (the leaf hash is the key: a transaction
 * set); d_select_words: ceil(n / 64) words in the accept bitmaps' layout, or NULL (all rows): only
 * rows whose bit is 1 are in the map, so the verify's bitmap can be passed as it is; d_root: 32
 * bytes; d_counts: 4 x uint32 or NULL: [0] distinct items, [1] selected rows dropped as duplicates
 * of a key, [2] inner nodes hashed, [3] the deepest inner node's depth.
 * DUPLICATES: among selected rows with equal keys the lowest row index supplies the leaf hash
 * (SHAMap::addItem refuses the second).  n == 0, or nothing selected: a zero root, zero counts.
 * DEFERRED ROWS: the blob calls write a zero ID for a row they defer (STL_TX_DEFERRED), and a
 * malformed row's ID is not written at all: before d_id of a blob call is passed as d_key, supply
 * those rows' IDs or clear their select bits -- the accept bitmap does the latter.
 * Before any device work: a NULL d_root, a NULL d_key with n > 0, n > STL_SHAMAP_MAX_ITEMS, d_key
 * or d_leaf_hash not 16-byte aligned, d_root or d_counts not 4-byte aligned is STL_EINVAL.  Runs on
 * the calling thread's current device.  A failure is a negative code; the outputs are written by
 * the call's last kernel alone, so a call that failed has not written them.
 * SYNCHRONISATION: none.  The call enqueues a fixed sequence on `stream` -- four 64-bit radix sort
 * passes (a fifth of one bit with a select bitmap), a scan, 64 level launches of which those
 * without a node at their depth return at once -- and returns; every count stays on the device.
 * MEMORY: the stream context holds the workspace, 89 B per row (16 B sort words, 8 B row numbers,
 * 1 B neighbour byte, 32 B sorted key, 32 B hash slot) plus the sort's temporary storage (what
 * rocPRIM asks for n rows, whatever the keys: 8 KB at 2^20 rows, 2 MB at 2^24) and 512 B; nothing
 * is sized by the number of inner nodes, which adversarial keys push to 63 (n - 1) + 1.
 * With stl_set_phase_timing on, a call's sort, heads-and-neighbours, level and finish times are
 * added to stl_stats.phase_ns[0..3] as one chunk. */
#define STL_SHAMAP_MAX_ITEMS 16777216u
int stl_shamap_root_device(const uint8_t *d_key, const uint8_t *d_leaf_hash, const uint64_t *d_select_words,
                           size_t n, uint8_t *d_root, uint32_t *d_counts, void *stream);
/* Host form: host memory (any alignment), synchronous: upload, the device form, 32 + 16 bytes back.
 * select_bitmap: ceil(n / 8) bytes, bit i of byte i / 8, or NULL; counts: nullable. */
int stl_shamap_root(const uint8_t *key, const uint8_t *leaf_hash, const uint8_t *select_bitmap, size_t n,
                    uint8_t root[32], uint32_t counts[4]);

/* ---- resident SHAMap: a state tree's root from each ledger's changes ----
 * The state tree lives from ledger to ledger and holds millions of entries, of which a ledger
 * changes a few thousand (Ledger::writeBack -> addGiveItem / updateGiveItem, Ledger.cpp:1228-1237;
 * delItem, SHAMap.cpp:685); the node keeps the map in memory and rehashes only the paths it has
 * touched (Ledger::updateHash, Ledger.cpp:273).  A stl_shamap_tree is the device-resident
 * counterpart: the tree's distinct keys and leaf hashes, sorted, in device memory from one call to
 * the next.  stl_shamap_tree_apply_device merges a batch of changes and leaves the new root in device
 * memory; only the buckets the batch touches -- a bucket is the keys that share their first 4
 * nibbles, 65,536 in all -- and the 4,369 nodes above the buckets are rehashed.
 * CONTRACT: after every successful call the root is what stl_shamap_root_device gives for the
 * tree's content, and the content is what the batches so far, read row by row, make of an empty map.
 *
 * A batch: d_key n * 32 bytes; d_leaf_hash n * 32 bytes, or NULL (the leaf hash is the key), not
 * read for a delete; d_op n bytes, 0: set (insert or replace), nonzero: delete, or NULL (every row
 * is a set).  The batch reads as a sequence of changes, like stl_acctdir_upsert: of rows with equal
 * keys the last one counts.  d_root: 32 bytes; d_counts: 8 x uint32 or NULL: [0] items after the
 * call, [1] inserted, [2] replaced, [3] deleted, [4] deletes of absent keys, [5] rows superseded by
 * a later row with the same key, [6] dirty buckets (those that hold a change's key), [7] leaves
 * gathered for rehashing (the items of the dirty buckets afterwards).  An apply to an empty tree is
 * how a tree is loaded.
 * Before any device work: a NULL tree, d_root, or d_key with n > 0, d_key or d_leaf_hash not 16-byte
 * aligned, d_root or d_counts not 4-byte aligned, n > capacity, a handle that is not live or a tree
 * of another device than the calling thread's is STL_EINVAL.  n == 0 is STL_OK and writes the
 * current root (counts: the items and seven zeros).
 * FAILURE: a call that returns a negative code leaves content, count and root as they were -- an
 * apply writes only the generation that is not live, and the host turns to it after the call's last
 * enqueue has succeeded; applying the same batch again then gives the right result.  The caller's
 * outputs are written by the call's last kernel alone.
 * CAPACITY AND SYNCHRONISATION: the ops are in device memory, so the host keeps an upper bound of
 * the count: the last count it has read plus the rows of every apply since.  While bound + n <=
 * capacity the call enqueues its fixed sequence on `stream` and returns without a host wait.
 * Otherwise it waits on `stream` once, behind the batch's sort and locate steps (which write work
 * areas alone), reads the exact count and the keys the batch inserts and deletes (20 bytes) and
 * resets the bound; if the count after the batch would exceed the capacity it is STL_ENOMEM and the
 * tree is unchanged -- so a full tree still takes replaces and deletes.  No kernel writes past the
 * capacity whatever the data.
 * COST: the merge moves every item into the other generation, O(items) bytes per apply (128 MiB at
 * 2^20 items, read and written); the hashing is proportional to the dirty buckets.
 * MEMORY: 193 B per row of capacity -- two generations of key and leaf hash (128 B), the scratch the
 * dirty buckets' subtrees are hashed in (65 B: one bucket may hold everything) -- plus 5.9 MB of
 * bucket values and per-bucket words, and per row of the largest batch 80 B in the tree and 89 B in
 * the stream context's SHAMap workspace with the sort's temporary storage (as stl_shamap_root_device
 * states it; never below what 65,536 rows ask for).
 * Concurrency: calls on one tree are serialised by the caller, and a call on another stream must be
 * ordered after the previous one by the caller; trees are independent of each other.  A tree lives
 * on the device current at creation; stl_shutdown frees every tree.  The previous generation stays
 * intact until the next apply.
 * With stl_set_phase_timing on, an apply's batch sort and locate, merge, subtree and top-and-finish
 * times are added to stl_stats.phase_ns[0..3] as one chunk. */
typedef struct stl_shamap_tree stl_shamap_tree;
typedef struct stl_shamap_tree_info {
  uint32_t struct_size; /* sizeof(stl_shamap_tree_info) */
  uint32_t capacity;
  uint32_t items;
  uint32_t bucket_depth; /* 4 */
  int32_t device;        /* HIP device ordinal */
  uint64_t bytes;        /* device memory the tree holds now */
  uint8_t root[32];
} stl_shamap_tree_info;
/* capacity in 1..STL_SHAMAP_MAX_ITEMS.  Synchronous.  STL_OK and *out (an empty tree: root zero),
 * or a negative code and *out = NULL. */
int stl_shamap_tree_create(uint32_t capacity, stl_shamap_tree **out);
/* Waits for the device, then frees the tree.  NULL, a destroyed handle and a handle from before
 * stl_shutdown are ignored.  No call on the tree may be running on another thread. */
void stl_shamap_tree_destroy(stl_shamap_tree *t);
/* Waits for the device; the exact item count and the root. */
int stl_shamap_tree_get_info(stl_shamap_tree *t, stl_shamap_tree_info *out);
int stl_shamap_tree_apply_device(stl_shamap_tree *t, const uint8_t *d_key, const uint8_t *d_leaf_hash,
                                 const uint8_t *d_op, size_t n, uint8_t *d_root, uint32_t *d_counts, void *stream);
/* Host form: host memory (any alignment), synchronous: upload, the device form, 32 + 32 bytes back. */
int stl_shamap_tree_apply(stl_shamap_tree *t, const uint8_t *key, const uint8_t *leaf_hash, const uint8_t *op,
                          size_t n, uint8_t root[32], uint32_t counts[8]);
/* d_root (32 bytes, 4-byte aligned) <- the current root; asynchronous on `stream`. */
int stl_shamap_tree_root_device(stl_shamap_tree *t, uint8_t *d_root, void *stream);
/* The sorted content: d_key and d_leaf_hash (rows * 32 bytes each, 16-byte aligned, either may be
 * NULL) <- the keys in memcmp order and their leaf hashes, *d_items (nullable) <- the item count;
 * asynchronous on `stream`.  rows must be at least the host's bound of the count (see CAPACITY; the
 * capacity always serves, and after stl_shamap_tree_get_info the bound is the count), else STL_EINVAL. */
int stl_shamap_tree_export_device(stl_shamap_tree *t, uint8_t *d_key, uint8_t *d_leaf_hash, size_t rows,
                                  uint32_t *d_items, void *stream);

/* ---- SHAMap inner nodes: what flushDirty writes, per set and per apply ----
 * Right after applyTransactions a node flushes both maps (LedgerConsensus.cpp:993-996 -> flushDirty,
 * SHAMap.cpp:972): every inner node the ledger changed goes to the node store, keyed by its hash,
 * its body "MIN\0" followed by the 16 child hashes (SHAMapTreeNode::addRaw, snfPREFIX); the same 512
 * bytes are what a peer acquiring a set or a ledger asks for (getNodeFat, getFetchPack).  The two
 * calls below are stl_shamap_root_device and stl_shamap_tree_apply_device -- the same root, counts,
 * duplicate rule, capacity rule, failure contract and argument checks -- and also write the inner
 * nodes they hash on the way.  Leaf nodes are the caller's: it holds the leaf blobs, and a node's
 * leaf mask tells which of its child hashes are leaf hashes.
 *
 * stl_shamap_nodes_device writes every inner node of the map exactly once: *count == counts[2].
 * stl_shamap_tree_apply_nodes_device writes the set E of the NEW tree's inner nodes, each once.  With
 * the dirty buckets those that hold the key of any row of the batch (counts[6]), E is every inner
 * node at depth >= 4 whose first four nibbles are a dirty bucket, and every inner node at depth < 4
 * (the root whenever the new tree holds a key) whose prefix is a prefix of a dirty bucket.
 * GUARANTEE: every inner node of the new tree whose hash is not the hash of an inner node of the old
 * tree is in E -- such a node has a changed key beneath it.  E may also hold unchanged nodes of dirty
 * buckets; a node store keyed by hash drops those.  With n == 0, *count = 0.
 * ORDER: the order of the rows is unspecified and may differ from run to run.
 * OVERFLOW: rows are written only at indices < max_nodes.  When *count > max_nodes the arrays hold
 * some max_nodes of the nodes and root and counts are still right; the caller then calls again with
 * room -- for a tree, stl_shamap_tree_export_device followed by stl_shamap_nodes_device.  A map of m
 * keys has at most 63 (m - 1) + 1 inner nodes.  No kernel stores past max_nodes rows whatever the data.
 * FAILURE: *count is written by the call's last kernel alone (for n == 0 of the set call, by a
 * memset as root and counts are); the four arrays may be partly written by a call that fails.  A tree
 * is unchanged by a failed call.
 * Before any device work, besides the checks of the calls they extend: a NULL out, hash, body or
 * count, a struct_size other than sizeof(stl_shamap_nodes_out), max_nodes > STL_SHAMAP_MAX_NODES,
 * and in the device form hash, body or id not 16-byte aligned or meta or count not 4-byte aligned
 * is STL_EINVAL.
 * SYNCHRONISATION: the device forms wait where the calls they extend wait, nowhere else.  The host
 * forms stage max_nodes * 580 bytes on the device, wait once for the count (4 bytes) and copy back
 * min(*count, max_nodes) rows; a host array may have any alignment. */
#define STL_SHAMAP_MAX_NODES 0xffffffc0u
#define STL_SHAMAP_NODE_BODY_BYTES 512u
typedef struct stl_shamap_nodes_out {
  uint32_t struct_size; /* sizeof(stl_shamap_nodes_out) */
  uint32_t max_nodes;   /* rows the four arrays have room for */
  uint8_t *hash;        /* max_nodes * 32: the node's hash = its node-store key */
  uint8_t *body;        /* max_nodes * 512: child hashes 0..15, zeros for an empty branch;
                           "MIN\0" || body is the snfPREFIX blob, SHA512Half of it = hash */
  uint8_t *id;          /* max_nodes * 32 or NULL: the key's first `depth` nibbles, rest 0
                           (SHAMapNodeID's masked key) */
  uint32_t *meta;       /* max_nodes or NULL: bits 0-7 depth (0..63), bits 8-15 zero,
                           bit 16+c set = branch c is a leaf (non-empty and holding one key) */
  uint32_t *count;      /* one word, required: nodes the call produced, may exceed max_nodes */
} stl_shamap_nodes_out;
int stl_shamap_nodes_device(const uint8_t *d_key, const uint8_t *d_leaf_hash, const uint64_t *d_select_words,
                            size_t n, uint8_t *d_root, uint32_t *d_counts, const stl_shamap_nodes_out *out,
                            void *stream);
int stl_shamap_nodes(const uint8_t *key, const uint8_t *leaf_hash, const uint8_t *select_bitmap, size_t n,
                     uint8_t root[32], uint32_t counts[4], const stl_shamap_nodes_out *out);
int stl_shamap_tree_apply_nodes_device(stl_shamap_tree *t, const uint8_t *d_key, const uint8_t *d_leaf_hash,
                                       const uint8_t *d_op, size_t n, uint8_t *d_root, uint32_t *d_counts,
                                       const stl_shamap_nodes_out *out, void *stream);
int stl_shamap_tree_apply_nodes(stl_shamap_tree *t, const uint8_t *key, const uint8_t *leaf_hash, const uint8_t *op,
                                size_t n, uint8_t root[32], uint32_t counts[8], const stl_shamap_nodes_out *out);

/* ---- resident SHAMap: hasItem, the item's hash and SHAMap::compare ----
 * The node asks its maps all the time: applyTransactions drops a candidate the closed ledger already
 * holds (hasTransaction, LedgerConsensus.cpp:1950), every disputed transaction is voted on per peer
 * with set->hasItem(txID) (LedgerConsensus.cpp:853, 1319-1359), and createDisputes runs SHAMap::compare
 * between our set and each peer's (LedgerConsensus.cpp:1263, SHAMapDelta.cpp:120).  The two calls
 * below answer from a stl_shamap_tree where it lies.  Both only read: content, count and root of a
 * tree are never changed by them, whatever they return.
 *
 * LOOKUP.  d_key: n * 32 bytes, 16-byte aligned.  d_found_words (required): ceil(n / 64) words in the
 * accept bitmaps' layout, bit i set when key i is in the tree; the words are written whole and the
 * last word's tail bits are zero (as stl_sigcache_lookup_device), so they combine with an accept
 * bitmap into a select bitmap (candidates = accept & ~found).  d_leaf_hash (n * 32 bytes, 16-byte
 * aligned, or NULL): the item's leaf hash, zeros for an absent key.  d_position (n words or NULL): the
 * key's row in stl_shamap_tree_export_device's order, or 0xFFFFFFFF; valid until the next apply.
 * Exactly those bytes are written; repeated keys are answered independently.  The item count is read
 * on the device; one lane per key bisects the range of the key's bucket alone (its begin from a scan
 * of the generation's 65,536 bucket counts, made per call).
 * Before any device work: a NULL tree, a NULL d_found_words or d_key with n > 0, d_key or d_leaf_hash
 * not 16-byte aligned, d_found_words not 8-byte or d_position not 4-byte aligned, n > 0xffffffc0, a
 * handle that is not live or a tree of another device than the calling thread's is STL_EINVAL.
 * n == 0 is STL_OK and writes nothing.
 * MEMORY: 256 KiB of bucket begin positions and the scan's temporary storage in the stream context;
 * nothing per key.
 *
 * COMPARE.  Let D be the differences of the two trees' contents: a key in exactly one tree, or in
 * both with different leaf hashes.  The rows are D in ascending key order (memcmp order, the order
 * of the reference's Delta map), truncated to the first max_rows; counts[0] is |D| whatever max_rows
 * is.  SHAMap::compare returns false once it has counted maxCount differences: counts[0] >= max_rows
 * is that condition -- but the rows here are the first ones in key order, not an unspecified part.
 * No store goes past max_rows rows whatever the data.  a == b is allowed: no difference.
 * BUCKET RULE (the reference's own assumption): a bucket -- the keys that share their first 4
 * nibbles -- whose (count, hash) is equal in both trees is taken as equal and not examined, as
 * SHAMap::compare does not descend into a branch with equal hashes.  That is exact when a leaf hash
 * commits to its key, which every SHAMap leaf kind does ("MLN\0" || data || index, "SND\0" || ... ||
 * id, and leaf = key for tnTRANSACTION_NM); leaf hashes that did not could hide a difference, here as
 * there.  counts[4] and counts[5] say what was examined: the cost follows what
 * differs, not what the trees hold.
 * Before any device work: a NULL tree, out or counts, a struct_size other than
 * sizeof(stl_shamap_diff_out), max_rows > STL_SHAMAP_MAX_NODES, max_rows > 0 with a NULL key or kind,
 * in the device form key, leaf_a or leaf_b not 16-byte aligned or counts not 4-byte aligned, trees of
 * different devices or of another device than the calling thread's, or a handle that is not live is
 * STL_EINVAL.
 * FAILURE: counts is written by the call's last kernel alone, so a call that failed has not written
 * it; the row arrays may be partly written.
 * MEMORY: 16 B per slot in the stream context -- a slot per item the host's bounds of the two counts
 * admit (see CAPACITY above) -- plus 1 MiB of per-bucket words and the scans' temporary storage.
 * The host form stages min(max_rows, slots) * 97 bytes on the device, waits once for counts[0] and
 * copies back min(counts[0], max_rows) rows; a host array may have any alignment.
 *
 * Both device forms are asynchronous on `stream` and never wait on the host; the host forms are
 * synchronous: upload, the device form, copy back.
 * Concurrency: lookups and compares only read trees and may run concurrently with each other, on
 * any streams.  With respect to an apply on the same tree the caller orders them, as it orders
 * applies: they read the generation that is live when they are called. */
int stl_shamap_tree_lookup_device(stl_shamap_tree *t, const uint8_t *d_key, size_t n, uint64_t *d_found_words,
                                  uint8_t *d_leaf_hash, uint32_t *d_position, void *stream);
/* found_bitmap: ceil(n / 8) bytes, bit i of byte i / 8. */
int stl_shamap_tree_lookup(stl_shamap_tree *t, const uint8_t *key, size_t n, uint8_t *found_bitmap,
                           uint8_t *leaf_hash, uint32_t *position);
#define STL_SHAMAP_DIFF_A_ONLY 1u  /* DeltaItem (item, null) */
#define STL_SHAMAP_DIFF_B_ONLY 2u  /* DeltaItem (null, item) */
#define STL_SHAMAP_DIFF_CHANGED 3u /* in both, leaf hashes differ */
typedef struct stl_shamap_diff_out {
  uint32_t struct_size; /* sizeof(stl_shamap_diff_out) */
  uint32_t max_rows;    /* rows the arrays have room for (the reference's maxCount) */
  uint8_t *key;         /* max_rows * 32, required unless max_rows == 0 */
  uint8_t *kind;        /* max_rows bytes, required unless max_rows == 0: STL_SHAMAP_DIFF_* */
  uint8_t *leaf_a;      /* max_rows * 32 or NULL: the item's leaf hash in a, zeros for B_ONLY */
  uint8_t *leaf_b;      /* max_rows * 32 or NULL: ... in b, zeros for A_ONLY */
  uint32_t *counts;     /* 8 words, required: [0] differences (may exceed max_rows), [1] A_ONLY,
                           [2] B_ONLY, [3] CHANGED, [4] buckets examined, [5] items examined
                           (those buckets' items of a plus of b), [6] items of a, [7] items of b */
} stl_shamap_diff_out;
int stl_shamap_tree_compare_device(stl_shamap_tree *a, stl_shamap_tree *b, const stl_shamap_diff_out *out,
                                   void *stream);
int stl_shamap_tree_compare(stl_shamap_tree *a, stl_shamap_tree *b, const stl_shamap_diff_out *out);

/* ---- resident SHAMap: SHAMap::snapShot as a fork into another handle, and a one-step revert ----
 * The reference starts every new ledger from prevLedger.mAccountStateMap->snapShot(true)
 * (Ledger.cpp:153) and every changed position from mAcquired[...]->snapShot(true)
 * (LedgerConsensus.cpp:1565-1591): the map it started from stays as it was.  A fork is that step for
 * resident trees: the apply reads one generation and writes another, and here the other generation
 * belongs to a different tree.
 * FORK: after a successful call dst holds src's content with the batch applied.  The batch follows
 * stl_shamap_tree_apply_device's rules (set or delete per row, the last of equal keys counts,
 * d_leaf_hash NULL: the leaf hash is the key); d_root and the eight d_counts are what that apply on
 * src would have written; dst's root, bucket values and count are those of its new content
 * (stl_shamap_root_device over dst's export gives the same root).  Whatever dst held before is
 * replaced -- and is what a revert of dst brings back.
 * src IS ONLY READ: its content, count, root, bucket values and revert state are unchanged; neither
 * of its generations and none of its work areas is written (every work area is dst's or the stream
 * context's), so forks of one src into different dsts on different streams may run at the same
 * time.  As with lookup and compare, the caller orders a fork against applies to src.
 * n == 0 IS THE PLAIN SNAPSHOT: dst becomes a copy of src.  Nothing is hashed or sorted: the rows
 * (by the count on the device, not the capacity), the 65,536 bucket values and the meta words are
 * copied by one kernel; the outputs are those of an apply of no rows to src.
 * CAPACITIES MAY DIFFER: dst only has to hold the result.  While src's host bound + n <= dst's
 * capacity the call enqueues and returns without a wait; otherwise it takes the apply's one-wait
 * path (the exact count of src, what the batch inserts and deletes), and if the result would not
 * fit dst it is STL_ENOMEM and both trees stay as they were.  Every read of src's rows is clamped
 * by min(count on the device, src's capacity), every store guarded by dst's capacity.
 * Before any device work: the apply's checks (on dst: n > dst's capacity is STL_EINVAL); src NULL
 * or src == dst, a handle that is not live, two trees of different devices or not of the calling
 * thread's device are STL_EINVAL.
 * FAILURE: a negative return leaves dst's content, count and root as they were (the live generation
 * is never written; the device forms commit after the last enqueue, the host forms once the results
 * are back) and src is never changed.  The caller's outputs are written by the last launch alone.
 * The _nodes forms are stl_shamap_tree_apply_nodes[_device] with src as the old tree: the rows are
 * the nodes of the dirty buckets and of the prefixes above them in dst's new tree, numbered, counted
 * and cut off at max_nodes in the same way; n == 0 stores no node and writes a count of zero.  The
 * normal close is one such call: fork the closed ledger's state into the next ledger's tree and hand
 * the new nodes to the node store.
 *
 * REVERT: stl_shamap_tree_revert(t) makes t what it was before the last successful apply or fork
 * into it -- content, count, root and bucket values -- by turning the host back to the previous
 * generation and to the host bound that went with it: no device work, no wait; the caller orders it
 * like an apply.  One step only: STL_EINVAL on a tree that has taken no apply, directly after a
 * revert, and after any apply or fork into t that returned a negative code past its argument checks
 * (that call may have half written the very generation a revert would turn to) until the next
 * successful one.  An apply of no rows changes nothing, this included.  Positions from earlier
 * lookups are invalid after a revert, as after an apply. */
int stl_shamap_tree_fork_device(stl_shamap_tree *src, stl_shamap_tree *dst, const uint8_t *d_key,
                                const uint8_t *d_leaf_hash, const uint8_t *d_op, size_t n, uint8_t *d_root,
                                uint32_t *d_counts, void *stream);
int stl_shamap_tree_fork(stl_shamap_tree *src, stl_shamap_tree *dst, const uint8_t *key, const uint8_t *leaf_hash,
                         const uint8_t *op, size_t n, uint8_t root[32], uint32_t counts[8]);
int stl_shamap_tree_fork_nodes_device(stl_shamap_tree *src, stl_shamap_tree *dst, const uint8_t *d_key,
                                      const uint8_t *d_leaf_hash, const uint8_t *d_op, size_t n, uint8_t *d_root,
                                      uint32_t *d_counts, const stl_shamap_nodes_out *out, void *stream);
int stl_shamap_tree_fork_nodes(stl_shamap_tree *src, stl_shamap_tree *dst, const uint8_t *key,
                               const uint8_t *leaf_hash, const uint8_t *op, size_t n, uint8_t root[32],
                               uint32_t counts[8], const stl_shamap_nodes_out *out);
int stl_shamap_tree_revert(stl_shamap_tree *t);

/* ---- resident SHAMap: SHAMap::getFetchPack between two trees ----
 * For every peer that is catching up the reference walks back ledger by ledger and asks
 * wantLedger's state map for getFetchPack(haveLedger's state map, ...) and its transaction map for
 * getFetchPack(nullptr, ...) (NetworkOPs.cpp:2799-2826, SHAMapSync.cpp:609-674).  The call below is
 * that walk's inner nodes for two resident trees.
 * THE PACK F of `want` against `have`: every inner node of want, at its SHAMapNodeID (depth, the
 * key's first `depth` nibbles), for which have holds no inner node at the same ID with the same
 * hash.  That is the set the reference's walk visits: it emits a node and descends into an inner
 * child only when !have->hasInnerNode(childID, childHash), hasInnerNode descends have by the ID and
 * compares the hash it finds there (SHAMapSync.cpp:552-570), and a node that differs makes its
 * parent differ.  The test is by position: a node of want whose hash have holds at another ID is in
 * F.  have NULL or empty: F is every inner node of want.  Equal roots, want == have (allowed) or an
 * empty want: F is empty.
 * LEAVES are not rows of this call: the leaves of a fetch pack (!have->hasLeafNode(tag, hash)) are
 * the rows of kind STL_SHAMAP_DIFF_A_ONLY and STL_SHAMAP_DIFF_CHANGED of
 * stl_shamap_tree_compare_device(want, have), and with have NULL want's export.
 * OUTPUTS: `out` as stl_shamap_nodes_device fills it -- hash, the 512-byte body, the optional id and
 * meta word (depth and leaf mask) -- each node of F once, at an index below max_nodes only, in no
 * particular order; *out->count = |F| whatever max_nodes is (the reference stops after `max` nodes
 * in walk order; here the caller sees how much room a second call needs).  counts (8 words; the
 * device form's d_counts may be NULL): [0] |F|, [1] buckets examined, [2] items of want gathered,
 * [3] items of have gathered, [4] inner nodes of want hashed as candidates, at all depths,
 * [5] candidates left out because have holds them ([4] - [5] == [0]), [6] items of want, [7] items
 * of have (0 for NULL).
 * READ-ONLY: content, count, root, host bound and revert state of both trees are unchanged whatever
 * the call returns, and so are their work areas: everything the call writes besides the caller's
 * arrays is the stream context's.  It may run beside lookups, compares and other fetch packs of the
 * same trees on any streams; against an apply or a fork into either tree the caller orders it.
 * BUCKET RULE, as the compare's: a bucket whose (count, hash) is equal in both trees is not
 * examined -- exact when leaf hashes commit to their keys, the assumption the reference makes when
 * it does not descend below an equal hash.  The cost follows what differs: the keys of the
 * differing buckets of both trees are gathered and hashed level by level, have's depth d just
 * before want's asks for it, and the 4,369 prefixes above the buckets are folded for both trees.
 * The device form is asynchronous on `stream` and never waits on the host: every count is read on
 * the device, grids and workspace come from the host's bounds of the two item counts.  The host
 * form stages max_nodes * 580 bytes on the device, waits once for the count and copies back
 * min(count, max_nodes) rows; a host array may have any alignment.
 * FAILURE: *out->count and counts are written by the call's last kernel alone, so a call that
 * failed has not written them; the row arrays may be partly written.
 * Before any device work: what the node-storing calls refuse in `out`; a NULL want; a handle that
 * is not live; trees of different devices or of another device than the calling thread's; d_counts
 * not 4-byte aligned is STL_EINVAL.
 * MEMORY: in the stream context 65 B per item of want's host bound plus 65 B per item of have's,
 * 1.5 MiB of per-bucket words, both trees' 4,369 top values and the scans' temporary storage.
 * Nothing is sized by the number of nodes.
 * With stl_set_phase_timing on the call adds to stl_stats.phase_ns[0..2]: buckets and gather, the
 * levels, top and finish. */
int stl_shamap_tree_fetch_pack_device(stl_shamap_tree *want, stl_shamap_tree *have,
                                      const stl_shamap_nodes_out *out, uint32_t *d_counts, void *stream);
int stl_shamap_tree_fetch_pack(stl_shamap_tree *want, stl_shamap_tree *have, const stl_shamap_nodes_out *out,
                               uint32_t counts[8]);

/* ---- resident SHAMap: SHAMap::getNodeFat and SHAMap::getPath by node ID ----
 * A peer that acquires a ledger or a transaction set asks with TMGetLedger (liTX_NODE / liAS_NODE),
 * and for every node ID of the packet the reference calls map->getNodeFat(id, nodeIDs, rawNodes,
 * fatRoot, fatLeaves) (PeerImp.cpp:597-650, SHAMapSync.cpp:231-306): a walk by (depth, masked key),
 * which a node store keyed by hash cannot make.  SHAMap::getPath / getTrustedPath
 * (SHAMap.cpp:1079-1109) is the same question asked by key.  The call below answers n such requests,
 * n <= STL_SHAMAP_GET_MAX_REQUESTS, from a stl_shamap_tree where it lies.
 * REQUESTS: d_id n * 32 bytes, 16-byte aligned; d_depth n bytes; d_mode n bytes or NULL (every
 * request STL_SHAMAP_GET_FAT).  NODE: the node at (depth, id) alone -- getNodeFat of the root with
 * fatRoot false, and hasNode.  FAT: what getNodeFat emits with fatRoot true.  PATH: getPath(id); id
 * is a full key and depth is not read.
 * THE NODE AT (depth, id): with [lo, hi) the tree's keys whose first `depth` nibbles are id's and
 * c = hi - lo, it is an inner node when c >= 2 or depth == 0 && c == 1; a leaf when c == 1,
 * depth >= 1 and (depth == 1 or the range one nibble shorter holds two keys or more); the empty root
 * when depth == 0 && c == 0; else absent.  An id with a bit set past its first `depth` nibbles is
 * absent: the wire constructor does not mask, and the reference's nodeID != wanted then fails.
 * ANSWERS, n entries each: d_status (bytes) STL_SHAMAP_AT_*; d_first and d_rows (words): the
 * request's node rows are [first, first + rows), first the exclusive prefix sum of rows in request
 * order; d_leaf_key and d_leaf_hash (n * 32 bytes, 16-byte aligned, or NULL): for AT_LEAF and
 * AT_OTHER_LEAF the leaf's key and leaf hash, zeros otherwise.
 * ROWS go into `out` as the node-storing calls fill it (hash, 512-byte body, optional id, optional
 * meta with depth and leaf mask), here in a fixed order.  A leaf has no row.  NODE on an inner node:
 * one row.  FAT on an inner node: with L the leading nibbles the range's first and last key share
 * (depth <= L <= 63), the inner nodes along id at depths depth .. L -- the chain of nodes with a
 * single, inner branch that the reference's do-while follows -- and then the inner children of the
 * node at L in branch order; leaf children are no rows, the node's leaf mask and body name them
 * (fatLeaves) and the caller's node store holds the blobs; the root of a one-key tree is one row.
 * PATH: the inner nodes along the key at depths 0 .. D - 1 in depth order (getPath's vector order,
 * getTrustedPath's reversed), D the first depth at which fewer than two keys share the key's prefix
 * and at least 1 in a tree that holds a key; what sits at depth D is AT_LEAF (the key), AT_OTHER_LEAF
 * (another key: its key is given, the proof of absence) or AT_ABSENT (an empty branch), and the rows
 * are written in all three cases.  An empty tree: no row, AT_ABSENT.  No request has more than 80
 * rows.  Requests are answered independently: a node two requests want is stored once for each.
 * *out->count is the sum of rows whatever max_nodes is; nothing is stored at an index >= max_nodes.
 * d_counts (8 words, or NULL): [0] the sum of rows, [1] requests AT_INNER, [2] AT_LEAF or
 * AT_OTHER_LEAF, [3] every other status, [4] buckets gathered, [5] items gathered, [6] distinct
 * nodes among the rows stored, [7] items of the tree.
 * READ-ONLY: content, count, root, host bound, revert state and work areas of the tree are unchanged
 * whatever the call returns; everything written besides the caller's arrays is the stream
 * context's.  It may run beside lookups, compares, fetch packs and other such calls on any streams;
 * against an apply or a fork into the tree the caller orders it.
 * The device form is asynchronous on `stream` and never waits on the host.  The cost follows the
 * requests: only the buckets that hold a wanted node at depth >= 4 are gathered and hashed level by
 * level, and the 4,369 prefixes above the buckets are folded once.  The 60 level launches run
 * whatever the requests are: one request costs what the launches cost.  The host form takes arrays
 * of any alignment, stages through the device's buffers, waits once for the count and copies back
 * min(count, max_nodes) rows.
 * FAILURE: *out->count and d_counts are written by the call's last launch alone; the per-request
 * arrays and the rows may be partly written by a call that fails.
 * Before any device work: what the node-storing calls refuse in `out`; a NULL tree; a handle that
 * is not live; a tree of another device than the calling thread's; with n > 0 a NULL d_id, d_depth,
 * d_status, d_first or d_rows; d_id, d_leaf_key or d_leaf_hash not 16-byte aligned, d_first, d_rows
 * or d_counts not 4-byte aligned; n > STL_SHAMAP_GET_MAX_REQUESTS is STL_EINVAL.  n == 0 is STL_OK:
 * *count = 0 and zero counts, nothing else.
 * MEMORY: in the stream context 73 B per item of the tree's host bound, 5 B per task
 * (min(80 n, max_nodes)), 1 MiB of per-bucket words, the 4,369 top values and the scans' temporary
 * storage.  Nothing is sized by the tree's node count.
 * With stl_set_phase_timing on the call adds to stl_stats.phase_ns[0..2]: ranges, tasks and gather;
 * the levels; top and finish. */
#define STL_SHAMAP_GET_MAX_REQUESTS 16777216u
#define STL_SHAMAP_GET_NODE 0u
#define STL_SHAMAP_GET_FAT 1u
#define STL_SHAMAP_GET_PATH 2u
#define STL_SHAMAP_AT_ABSENT 0u     /* "Peer requested node not in map"; PATH: an empty branch */
#define STL_SHAMAP_AT_INNER 1u
#define STL_SHAMAP_AT_LEAF 2u
#define STL_SHAMAP_AT_EMPTY_ROOT 3u /* the root of an empty tree: getNodeFat returns false */
#define STL_SHAMAP_AT_INVALID 4u    /* depth > 63 (SHAMapNodeID::isValid), or an unknown mode */
#define STL_SHAMAP_AT_OTHER_LEAF 5u /* PATH only: the path ends at a leaf with another key */
int stl_shamap_tree_get_nodes_device(stl_shamap_tree *t, const uint8_t *d_id, const uint8_t *d_depth,
                                     const uint8_t *d_mode, size_t n, uint8_t *d_status, uint32_t *d_first,
                                     uint32_t *d_rows, uint8_t *d_leaf_key, uint8_t *d_leaf_hash,
                                     const stl_shamap_nodes_out *out, uint32_t *d_counts, void *stream);
int stl_shamap_tree_get_nodes(stl_shamap_tree *t, const uint8_t *id, const uint8_t *depth, const uint8_t *mode,
                              size_t n, uint8_t *status, uint32_t *first, uint32_t *rows, uint8_t *leaf_key,
                              uint8_t *leaf_hash, const stl_shamap_nodes_out *out, uint32_t counts[8]);

#ifdef __cplusplus
}
#endif

#endif /* STL_H */
