"""Python mirror of stellard's signature-check interface over libstl.

Reference interface being mirrored (hfeeki/stellard):
  * RippleAddress::verifySignature(uint256 const&, Blob const&)
      src/ripple_data/protocol/RippleAddress.cpp:190-200
      -> throws std::runtime_error("bad inputs to verifySignature") when the
         key is not 32 bytes or the signature not 64 bytes (:192-194);
         returns crypto_sign_verify_detached(...) == 0 && S < L.
  * StellarPublicKey::verifySignature  src/ripple_data/crypto/StellarPublicKey.cpp:67-77
  * SerializedTransaction::checkSign(const RippleAddress&)
      src/ripple_app/misc/SerializedTransaction.cpp:220-230 (any exception -> false)

Every call goes to the gfx950 kernels through the C ABI; nothing here
verifies on the CPU.
"""
import ctypes

import numpy as np

from . import _native as N

POLICY_SODIUM_1_0_18 = N.STL_POLICY_SODIUM_1_0_18
POLICY_STELLARD_1_0_0 = N.STL_POLICY_STELLARD_1_0_0
# OR into `policy` to check with full-length scalars (same bits, slower)
FULL_LENGTH = N.STL_FULL_LENGTH
# OR into `policy` to decode each distinct public key of a batch once
DEDUP_KEYS = N.STL_DEDUP_KEYS
ONE_LANE = N.STL_ONE_LANE
NO_AUTO_DEDUP = N.STL_NO_AUTO_DEDUP


class BadInputs(RuntimeError):
    """std::runtime_error("bad inputs to verifySignature") (RippleAddress.cpp:193)."""


def _buf(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# libsodium's crypto_sign_verify_detached signature (stl_verify_fn)
VERIFY_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_void_p)


class Config(ctypes.Structure):
    """stl_config (include/stl.h, ABI 3)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("device_count", ctypes.c_int32),
                ("first_device", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("shards_per_device", ctypes.c_int32), ("reserved", ctypes.c_uint32),
                ("fallback_verify", VERIFY_FN)]


_fallback_keepalive = []


def init(device_count=0, first_device=0, flags=0, shards_per_device=1, fallback_verify=None):
    """stl_init (sodium_init's place, ripple_app.cpp:129-132).  flags:
    N.STL_CFG_RCCL_GATHER / N.STL_CFG_NO_RCCL.  ``fallback_verify``: a
    VERIFY_FN (the caller's libsodium check) that stl_ed25519_verify_detached
    answers device failures with."""
    fb = fallback_verify if fallback_verify is not None else VERIFY_FN()
    if fallback_verify is not None:
        _fallback_keepalive.append(fallback_verify)  # libstl keeps the pointer
    cfg = Config(ctypes.sizeof(Config), device_count, first_device, flags, shards_per_device, 0, fb)
    return N.check(N.load().stl_init(ctypes.byref(cfg)), "stl_init")


def shutdown():
    N.load().stl_shutdown()


def shard_range(n, rank, world):
    """stl_shard_range: contiguous 64-aligned index shard of rank r."""
    lo, hi = ctypes.c_size_t(0), ctypes.c_size_t(0)
    N.load().stl_shard_range(n, rank, world, ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def shard_range_bytes(lens, rank, world):
    """stl_shard_range_bytes: byte-balanced 64-aligned shard of rank r."""
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    lo, hi = ctypes.c_size_t(0), ctypes.c_size_t(0)
    N.load().stl_shard_range_bytes(_buf(lens), lens.shape[0], rank, world, ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def verify_signature(hash32, sig, pk):
    """RippleAddress::verifySignature: bool, raises BadInputs on size mismatch."""
    pk, sig, hash32 = bytes(pk), bytes(sig), bytes(hash32)
    if len(pk) != 32 or len(sig) != 64:
        raise BadInputs("bad inputs to verifySignature")
    rc = N.load().stl_ed25519_verify_detached(sig, hash32, len(hash32), pk)
    if rc == 0:
        return True
    if rc == -1:
        return False
    raise N.StlError(rc, "stl_ed25519_verify_detached")


def crypto_sign_verify_detached(sig, m, pk):
    """libsodium call surface: 0 accept / -1 reject (+ stellard's S<L)."""
    sig, m, pk = bytes(sig), bytes(m), bytes(pk)
    if len(sig) != 64 or len(pk) != 32:
        return -1
    rc = N.load().stl_ed25519_verify_detached(sig, m, len(m), pk)
    if rc in (0, -1):
        return rc
    raise N.StlError(rc, "stl_ed25519_verify_detached")


def unpack_bitmap(bitmap, n):
    return np.unpackbits(np.frombuffer(bytes(bitmap), dtype=np.uint8), bitorder="little")[:n].astype(bool)


def verify_batch(sig, msg, pk, policy=POLICY_SODIUM_1_0_18):
    """Batch RippleAddress::verifySignature over host arrays -> bool[n]."""
    sig = np.ascontiguousarray(sig, dtype=np.uint8).reshape(-1, 64)
    msg = np.ascontiguousarray(msg, dtype=np.uint8).reshape(-1, 32)
    pk = np.ascontiguousarray(pk, dtype=np.uint8).reshape(-1, 32)
    n = sig.shape[0]
    if msg.shape[0] != n or pk.shape[0] != n:
        raise ValueError("sig/msg/pk batch sizes differ")
    bitmap = np.zeros((n + 7) // 8, dtype=np.uint8)
    N.check(N.load().stl_ed25519_verify_batch(_buf(sig), _buf(msg), _buf(pk), n, _buf(bitmap), policy),
            "stl_ed25519_verify_batch")
    return unpack_bitmap(bitmap, n)


def tx_verify_batch(preimages, sig, pk, policy=POLICY_SODIUM_1_0_18):
    """Batch checkSign: preimages is a list of bytes ("STX\\0" || fields)."""
    n = len(preimages)
    lens = np.array([len(p) for p in preimages], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    if n:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    blob = np.frombuffer(b"".join(bytes(p) for p in preimages) or b"\0", dtype=np.uint8).copy()
    sig = np.ascontiguousarray(sig, dtype=np.uint8).reshape(-1, 64)
    pk = np.ascontiguousarray(pk, dtype=np.uint8).reshape(-1, 32)
    bitmap = np.zeros((n + 7) // 8, dtype=np.uint8)
    N.check(N.load().stl_tx_verify_batch(_buf(blob), _buf(offs), _buf(lens), _buf(sig), _buf(pk), n,
                                         _buf(bitmap), policy), "stl_tx_verify_batch")
    return unpack_bitmap(bitmap, n)


def _pack(chunks):
    n = len(chunks)
    lens = np.array([len(p) for p in chunks], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    if n:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    buf = np.frombuffer(b"".join(bytes(p) for p in chunks) + b"\0" * 4, dtype=np.uint8).copy()
    return buf, offs, lens


TX_OK, TX_DEFERRED, TX_MALFORMED = N.STL_TX_OK, N.STL_TX_DEFERRED, N.STL_TX_MALFORMED


BLOB_TRANSACTION, BLOB_VALIDATION = N.STL_BLOB_TRANSACTION, N.STL_BLOB_VALIDATION


def signed_blob_verify_batch(blobs, kind=BLOB_TRANSACTION, policy=POLICY_SODIUM_1_0_18, ids=False):
    """stl_signed_blob_verify_batch: the signature check of serialized signed
    objects (list of bytes).  kind BLOB_TRANSACTION = checkSign,
    BLOB_VALIDATION = SerializedValidation::isValid.  Returns (accept bool[n],
    status uint8[n]) plus the IDs (n, 32) when ``ids``."""
    n = len(blobs)
    buf, offs, lens = _pack(blobs)
    bitmap = np.zeros((n + 7) // 8 or 1, dtype=np.uint8)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    idb = np.zeros((max(n, 1), 32), dtype=np.uint8) if ids else None
    N.check(N.load().stl_signed_blob_verify_batch(kind, _buf(buf), _buf(offs), _buf(lens), n, _buf(bitmap),
                                                  _buf(status), _buf(idb) if ids else None, policy),
            "stl_signed_blob_verify_batch")
    bits = unpack_bitmap(bitmap, n)
    return (bits, status[:n], idb[:n]) if ids else (bits, status[:n])


def tx_blob_verify_batch(blobs, policy=POLICY_SODIUM_1_0_18, tx_ids=False):
    """checkSign straight from serialized transactions (list of bytes, each
    the whole transaction with its TxnSignature).  Returns (accept bool[n],
    status uint8[n]) -- status TX_OK / TX_DEFERRED / TX_MALFORMED, see
    include/stl.h -- plus the transaction IDs (n, 32) when ``tx_ids``."""
    n = len(blobs)
    buf, offs, lens = _pack(blobs)
    bitmap = np.zeros((n + 7) // 8 or 1, dtype=np.uint8)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    ids = np.zeros((max(n, 1), 32), dtype=np.uint8) if tx_ids else None
    N.check(N.load().stl_tx_blob_verify_batch(_buf(buf), _buf(offs), _buf(lens), n, _buf(bitmap), _buf(status),
                                              _buf(ids) if tx_ids else None, policy), "stl_tx_blob_verify_batch")
    bits = unpack_bitmap(bitmap, n)
    return (bits, status[:n], ids[:n]) if tx_ids else (bits, status[:n])


def proposal_preimage(propose_seq, close_time, prev_ledger, position):
    """LedgerProposal::getSigningHash preimage (LedgerProposal.cpp:54-65):
    "PRP\0" || seq || closeTime (big-endian u32, Serializer::add32) ||
    previous ledger || position (uint256 bytes, add256); 76 bytes."""
    prev_ledger, position = bytes(prev_ledger), bytes(position)
    if len(prev_ledger) != 32 or len(position) != 32:
        raise ValueError("ledger hashes are 32 bytes")
    return (b"PRP\x00" + int(propose_seq).to_bytes(4, "big") + int(close_time).to_bytes(4, "big")
            + prev_ledger + position)


# ---- transaction level: SerializedTransaction::checkSign ----

class SignedTx:
    """The signature-check state of one SerializedTransaction.

    Mirrors src/ripple_app/misc/SerializedTransaction.cpp:192-230 and the
    cache flags of SerializedTransaction.h:116-131: ``signing_pub_key`` is the
    sfSigningPubKey VL field (any length), ``txn_signature`` the sfTxnSignature
    VL field (None when absent: getFieldVL returns an empty Blob,
    SerializedObject.cpp:814), ``preimage`` the signing preimage
    "STX\\0" || fields without TxnSignature (STObject::getSigningHash,
    SerializedObject.cpp:444-450)."""

    def __init__(self, signing_pub_key, txn_signature, preimage):
        self.signing_pub_key = bytes(signing_pub_key)
        self.txn_signature = None if txn_signature is None else bytes(txn_signature)
        self.preimage = bytes(preimage)
        self.sig_good = False   # mSigGood
        self.sig_bad = False    # mSigBad

    def well_formed(self):
        """verifySignature throws on a key that is not 32 bytes or a signature
        that is not 64 (RippleAddress.cpp:192-194); checkSign maps the throw to
        false (SerializedTransaction.cpp:211-217, 226-229)."""
        return len(self.signing_pub_key) == 32 and self.txn_signature is not None and len(self.txn_signature) == 64

    def set_good(self):
        self.sig_good = True

    def check_sign(self, policy=POLICY_SODIUM_1_0_18):
        """SerializedTransaction::checkSign(): cached verdict, else verify."""
        return check_sign_batch([self], policy=policy)[0]


def check_sign_batch(txs, policy=POLICY_SODIUM_1_0_18, mark="both"):
    """checkSign over many transactions with one stl_tx_verify_batch call.

    Cached rows return their verdict (mSigGood / mSigBad); malformed rows are
    rejected on the host and never reach the GPU.  ``mark="both"`` records
    both verdicts like the serial path; ``mark="good_only"`` records accepts
    only -- the ledger-close pre-verify, which must
    not call setBad() because LedgerConsensus.cpp:2101-2106 applies unflagged
    transactions without a signature check.  Returns a list of bools."""
    if mark not in ("both", "good_only"):
        raise ValueError("mark must be 'both' or 'good_only'")
    out = [False] * len(txs)
    todo = []
    for i, t in enumerate(txs):
        if t.sig_good:
            out[i] = True
        elif t.sig_bad:
            out[i] = False
        elif not t.well_formed():
            if mark == "both":
                t.sig_bad = True
        else:
            todo.append(i)
    if todo:
        sig = np.frombuffer(b"".join(txs[i].txn_signature for i in todo), np.uint8).reshape(-1, 64)
        pk = np.frombuffer(b"".join(txs[i].signing_pub_key for i in todo), np.uint8).reshape(-1, 32)
        bits = tx_verify_batch([txs[i].preimage for i in todo], sig, pk, policy=policy)
        for i, b in zip(todo, bits):
            out[i] = bool(b)
            if b:
                txs[i].sig_good = True
            elif mark == "both":
                txs[i].sig_bad = True
    return out


# ---- device-resident (torch tensors as HBM buffers; torch is plumbing only) ----

def _stream_ptr(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def verify_batch_device(sig, msg, pk, out_words=None, policy=POLICY_SODIUM_1_0_18, stream=None):
    """sig (n,64) / msg (n,32) / pk (n,32) uint8 CUDA tensors -> int64[ceil(n/64)]
    bitmap words (async on ``stream``)."""
    import torch
    n = sig.shape[0]
    if out_words is None:
        out_words = torch.empty((n + 63) // 64, dtype=torch.int64, device=sig.device)
    for t in (sig, msg, pk, out_words):
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("device entry point needs contiguous CUDA tensors")
    N.check(N.load().stl_ed25519_verify_batch_device(
        ctypes.c_void_p(sig.data_ptr()), ctypes.c_void_p(msg.data_ptr()), ctypes.c_void_p(pk.data_ptr()), n,
        ctypes.c_void_p(out_words.data_ptr()), policy, _stream_ptr(stream)), "stl_ed25519_verify_batch_device")
    return out_words


def tx_hash_batch_device(preimages, offsets, lengths, out_msg=None, stream=None):
    """SHA512Half of signing preimages already in HBM (uint8 / int64 / int32
    CUDA tensors; getSigningHash, SerializedObject.cpp:444-450) -> (n,32) uint8
    signing hashes, asynchronously on ``stream``; with verify_batch_device this
    is the device-resident checkSign (stl_tx_verify_batch)."""
    import torch
    n = offsets.shape[0]
    if out_msg is None:
        out_msg = torch.empty((n, 32), dtype=torch.uint8, device=preimages.device)
    for t in (preimages, offsets, lengths, out_msg):
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("device entry point needs contiguous CUDA tensors")
    if offsets.dtype != torch.int64 or lengths.dtype != torch.int32:
        raise ValueError("offsets must be int64 and lengths int32")
    N.check(N.load().stl_tx_hash_batch_device(
        ctypes.c_void_p(preimages.data_ptr()), ctypes.c_void_p(offsets.data_ptr()),
        ctypes.c_void_p(lengths.data_ptr()), n, ctypes.c_void_p(out_msg.data_ptr()), _stream_ptr(stream)),
        "stl_tx_hash_batch_device")
    return out_msg


def _check_rows(*ts):
    import torch
    for t in ts:
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise ValueError("device entry point needs contiguous CUDA tensors")
    if ts[1].dtype != torch.int64 or ts[2].dtype != torch.int32:
        raise ValueError("offsets must be int64 and lengths int32")


def tx_verify_batch_device(preimages, offsets, lengths, sig, pk, out_words=None, policy=POLICY_SODIUM_1_0_18,
                           stream=None):
    """stl_tx_verify_batch_device: the device-resident checkSign in one call --
    SHA512Half of each preimage and the verify, chunk by chunk over two
    streams -> int64 bitmap words (same bits as tx_hash_batch_device +
    verify_batch_device)."""
    import torch
    n = offsets.shape[0]
    if out_words is None:
        out_words = torch.empty(((n + 63) // 64,), dtype=torch.int64, device=preimages.device)
    _check_rows(preimages, offsets, lengths, sig, pk, out_words)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    N.check(N.load().stl_tx_verify_batch_device(p(preimages), p(offsets), p(lengths), p(sig), p(pk), n, p(out_words),
                                                policy, _stream_ptr(stream)), "stl_tx_verify_batch_device")
    return out_words


def signed_blob_verify_batch_device(blobs, offsets, lengths, out_words=None, tx_ids=False,
                                    policy=POLICY_SODIUM_1_0_18, stream=None, kind=None, out_status=None,
                                    out_ids=None):
    """stl_signed_blob_verify_batch_device: checkSign from serialized objects
    in HBM in one call -> dict of words (bitmap), status and (tx_ids or
    out_ids) tx_id."""
    import torch
    n = offsets.shape[0]
    dev = blobs.device
    if out_words is None:
        out_words = torch.empty(((n + 63) // 64,), dtype=torch.int64, device=dev)
    status = torch.empty((n,), dtype=torch.uint8, device=dev) if out_status is None else out_status
    tx_id = out_ids if out_ids is not None else (torch.empty((n, 32), dtype=torch.uint8, device=dev)
                                                 if tx_ids else None)
    # the kernels write raw bytes: a wider dtype would hold packed bytes the
    # caller misreads
    if status.dtype != torch.uint8 or (tx_id is not None and tx_id.dtype != torch.uint8):
        raise ValueError("out_status / out_ids must be torch.uint8")
    if tx_id is not None and tx_id.dim() > 1 and tx_id.shape[-1] != 32:
        raise ValueError("out_ids must be (n, 32) bytes")
    if status.numel() < n or (tx_id is not None and tx_id.numel() < 32 * n):
        raise ValueError("status / id buffers smaller than the batch")
    _check_rows(blobs, offsets, lengths, out_words, status, tx_id)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    N.check(N.load().stl_signed_blob_verify_batch_device(
        N.STL_BLOB_TRANSACTION if kind is None else kind, p(blobs), p(offsets), p(lengths), n, p(out_words),
        p(status), p(tx_id), policy, _stream_ptr(stream)), "stl_signed_blob_verify_batch_device")
    return {"words": out_words, "status": status, "tx_id": tx_id}


def tx_blob_prepare_device(blobs, offsets, lengths, tx_ids=True, stream=None, kind=None):
    """Serialized transactions already in HBM (uint8 / int64 / int32 CUDA
    tensors) -> dict of msg (n,32), sig (n,64), pk (n,32), status (n,) and
    tx_id (n,32) tensors, asynchronously on ``stream``; follow with
    verify_batch_device(sig, msg, pk)."""
    import torch
    n = offsets.shape[0]
    dev = blobs.device
    out = {"msg": torch.empty((n, 32), dtype=torch.uint8, device=dev),
           "sig": torch.empty((n, 64), dtype=torch.uint8, device=dev),
           "pk": torch.empty((n, 32), dtype=torch.uint8, device=dev),
           "status": torch.empty((n,), dtype=torch.uint8, device=dev),
           "tx_id": torch.empty((n, 32), dtype=torch.uint8, device=dev) if tx_ids else None}
    for t in (blobs, offsets, lengths):
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("device entry point needs contiguous CUDA tensors")
    if offsets.dtype != torch.int64 or lengths.dtype != torch.int32:
        raise ValueError("offsets must be int64 and lengths int32")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    N.check(N.load().stl_signed_blob_prepare_device(
        N.STL_BLOB_TRANSACTION if kind is None else kind, ptr(blobs), ptr(offsets), ptr(lengths), n,
        ptr(out["msg"]), ptr(out["sig"]), ptr(out["pk"]), ptr(out["tx_id"]), ptr(out["status"]),
        _stream_ptr(stream)), "stl_signed_blob_prepare_device")
    return out


# ---- signer authority: account IDs and the master-key match ----

ACCOUNT_ID_BYTES = N.STL_ACCOUNT_ID_BYTES
SIGNER_NOT_MASTER, SIGNER_MASTER, SIGNER_UNDECIDED = (N.STL_SIGNER_NOT_MASTER, N.STL_SIGNER_MASTER,
                                                      N.STL_SIGNER_UNDECIDED)


def _check_ids(n, **ts):
    """The kernels write raw bytes: every ID buffer is uint8 and (n, 20)."""
    import torch
    for name, t in ts.items():
        if t is None:
            continue
        if t.dtype != torch.uint8:
            raise ValueError(f"{name} must be torch.uint8")
        if tuple(t.shape) != (n, ACCOUNT_ID_BYTES):
            raise ValueError(f"{name} must be (n, 20) bytes")


def account_id_batch(pk):
    """stl_account_id_batch: Hash160 of n 32-byte account public keys (host
    memory; RippleAddress::getAccountID) -> (n, 20) uint8."""
    pk = np.ascontiguousarray(pk)
    if pk.dtype != np.uint8 or pk.ndim != 2 or pk.shape[1] != 32:
        raise ValueError("pk must be (n, 32) uint8")
    n = pk.shape[0]
    out = np.zeros((n, ACCOUNT_ID_BYTES), dtype=np.uint8)
    N.check(N.load().stl_account_id_batch(_buf(pk), n, _buf(out)), "stl_account_id_batch")
    return out


def account_id_batch_device(pk, out=None, stream=None):
    """pk (n, 32) uint8 CUDA tensor -> (n, 20) uint8 account IDs (async on
    ``stream``)."""
    import torch
    if pk.dtype != torch.uint8 or pk.dim() != 2 or pk.shape[1] != 32:
        raise ValueError("pk must be (n, 32) torch.uint8")
    n = pk.shape[0]
    if out is None:
        out = torch.empty((n, ACCOUNT_ID_BYTES), dtype=torch.uint8, device=pk.device)
    _check_ids(n, out=out)
    for t in (pk, out):
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("device entry point needs contiguous CUDA tensors")
    N.check(N.load().stl_account_id_batch_device(ctypes.c_void_p(pk.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
                                                 _stream_ptr(stream)), "stl_account_id_batch_device")
    return out


def tx_blob_signer_batch_device(blobs, offsets, lengths, accounts=True, stream=None, out_signer_id=None,
                                out_account=None, out_authority=None):
    """stl_tx_blob_signer_batch_device: serialized transactions in HBM (as
    tx_blob_prepare_device takes them) -> dict of signer_id (n, 20), account
    (n, 20), or None without ``accounts``, and authority (n,) -- SIGNER_MASTER
    / SIGNER_NOT_MASTER / SIGNER_UNDECIDED, see include/stl.h."""
    import torch
    n = offsets.shape[0]
    dev = blobs.device
    signer = torch.empty((n, ACCOUNT_ID_BYTES), dtype=torch.uint8, device=dev) if out_signer_id is None \
        else out_signer_id
    account = out_account if out_account is not None else (
        torch.empty((n, ACCOUNT_ID_BYTES), dtype=torch.uint8, device=dev) if accounts else None)
    authority = torch.empty((n,), dtype=torch.uint8, device=dev) if out_authority is None else out_authority
    _check_ids(n, out_signer_id=signer, out_account=account)
    if authority.dtype != torch.uint8 or tuple(authority.shape) != (n,):
        raise ValueError("out_authority must be (n,) torch.uint8")
    if blobs.dtype != torch.uint8:
        raise ValueError("blobs must be torch.uint8")
    _check_rows(blobs, offsets, lengths, signer, account, authority)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    N.check(N.load().stl_tx_blob_signer_batch_device(p(blobs), p(offsets), p(lengths), n, p(signer), p(account),
                                                     p(authority), _stream_ptr(stream)),
            "stl_tx_blob_signer_batch_device")
    return {"signer_id": signer, "account": account, "authority": authority}


def tx_blob_signer_batch(blobs, accounts=True):
    """stl_tx_blob_signer_batch: who signed each serialized transaction (list
    of bytes).  Returns (signer_id (n, 20), account (n, 20) or None, authority
    uint8[n])."""
    n = len(blobs)
    buf, offs, lens = _pack(blobs)
    signer = np.zeros((max(n, 1), ACCOUNT_ID_BYTES), dtype=np.uint8)
    account = np.zeros((max(n, 1), ACCOUNT_ID_BYTES), dtype=np.uint8) if accounts else None
    authority = np.zeros(max(n, 1), dtype=np.uint8)
    N.check(N.load().stl_tx_blob_signer_batch(_buf(buf), _buf(offs), _buf(lens), n, _buf(signer),
                                              _buf(account) if accounts else None, _buf(authority)),
            "stl_tx_blob_signer_batch")
    return signer[:n], (account[:n] if accounts else None), authority[:n]


# ---- account directory (stl_acctdir_*) ----

ACCT_HAS_REGULAR_KEY, ACCT_MASTER_DISABLED, ACCT_ABSENT, ACCT_NOT_FOUND = (
    N.STL_ACCT_HAS_REGULAR_KEY, N.STL_ACCT_MASTER_DISABLED, N.STL_ACCT_ABSENT, N.STL_ACCT_NOT_FOUND)
ACCTDIR_MAX_ACCOUNTS = N.STL_ACCTDIR_MAX_ACCOUNTS
(AUTH_MASTER, AUTH_REGULAR, AUTH_MASTER_DISABLED, AUTH_BAD_AUTH, AUTH_BAD_AUTH_MASTER, AUTH_NO_ACCOUNT,
 AUTH_UNDECIDED) = (N.STL_AUTH_MASTER, N.STL_AUTH_REGULAR, N.STL_AUTH_MASTER_DISABLED, N.STL_AUTH_BAD_AUTH,
                    N.STL_AUTH_BAD_AUTH_MASTER, N.STL_AUTH_NO_ACCOUNT, N.STL_AUTH_UNDECIDED)


class _DeviceObject:
    """A handle object of libstl that lives on one device (``_h``, made by the
    subclass's constructor): closing, use as a context manager, ``handle`` and
    ``info`` over ``<_prefix>_destroy`` / ``<_prefix>_get_info``."""
    _prefix, _Info = None, None
    _info_skip = ("struct_size",)

    def close(self):
        if self._h is not None:
            getattr(N.load(), self._prefix + "_destroy")(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    @property
    def handle(self):
        return self._h

    def info(self):
        i = self._Info(struct_size=ctypes.sizeof(self._Info))
        name = self._prefix + "_get_info"
        N.check(getattr(N.load(), name)(self._h, ctypes.byref(i)), name)
        return {k: getattr(i, k) for k, _ in self._Info._fields_ if k not in self._info_skip}


class AcctDirInfo(ctypes.Structure):
    """stl_acctdir_info (include/stl.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("capacity", ctypes.c_uint32), ("records", ctypes.c_uint32),
                ("slots", ctypes.c_uint32), ("longest_probe", ctypes.c_uint32), ("device", ctypes.c_int32),
                ("bytes", ctypes.c_uint64), ("seed", ctypes.c_uint64)]


class AccountDirectory(_DeviceObject):
    """A device-resident snapshot of the account-root fields Transactor::checkSig
    reads (stl_acctdir_create), keyed by account ID and updated per ledger with
    ``upsert``; ``tx_blob_authority_device`` gives checkSig's verdict (AUTH_*)
    per serialized transaction against the state as last upserted.

        with AccountDirectory(capacity) as d:
            d.upsert(ids, flags, regular_keys)
            out = d.tx_blob_authority_device(blobs, offsets, lengths)
    """

    _prefix, _Info = "stl_acctdir", AcctDirInfo

    def __init__(self, capacity, seed=0):
        h = ctypes.c_void_p()
        N.check(N.load().stl_acctdir_create(int(capacity), int(seed), ctypes.byref(h)), "stl_acctdir_create")
        self._h = h

    def upsert(self, account_id, flags, regular_key=None):
        """Host arrays: account_id (m, 20) uint8, flags (m,) uint8 of ACCT_*
        bits, regular_key (m, 20) uint8 (optional when no row has
        ACCT_HAS_REGULAR_KEY).  Synchronous; the last occurrence of an ID wins."""
        account_id = np.ascontiguousarray(account_id)
        flags = np.ascontiguousarray(flags)
        if account_id.dtype != np.uint8 or account_id.ndim != 2 or account_id.shape[1] != ACCOUNT_ID_BYTES:
            raise ValueError("account_id must be (m, 20) uint8")
        m = account_id.shape[0]
        if flags.dtype != np.uint8 or flags.shape != (m,):
            raise ValueError("flags must be (m,) uint8")
        if regular_key is not None:
            regular_key = np.ascontiguousarray(regular_key)
            if regular_key.dtype != np.uint8 or regular_key.shape != (m, ACCOUNT_ID_BYTES):
                raise ValueError("regular_key must be (m, 20) uint8")
        N.check(N.load().stl_acctdir_upsert(self._h, _buf(account_id), _buf(flags),
                                            _buf(regular_key) if regular_key is not None else None, m),
                "stl_acctdir_upsert")

    def lookup_device(self, account_id, regular_keys=True, stream=None, out_flags=None, out_regular_key=None):
        """account_id (n, 20) uint8 CUDA tensor -> dict of flags (n,) -- the
        ACCT_* bits, or ACCT_NOT_FOUND -- and regular_key (n, 20), or None
        without ``regular_keys`` (async on ``stream``)."""
        import torch
        if account_id.dtype != torch.uint8:
            raise ValueError("account_id must be torch.uint8")
        if account_id.dim() != 2 or account_id.shape[1] != ACCOUNT_ID_BYTES:
            raise ValueError("account_id must be (n, 20) bytes")
        n = account_id.shape[0]
        dev = account_id.device
        flags = torch.empty((n,), dtype=torch.uint8, device=dev) if out_flags is None else out_flags
        rk = out_regular_key if out_regular_key is not None else (
            torch.empty((n, ACCOUNT_ID_BYTES), dtype=torch.uint8, device=dev) if regular_keys else None)
        _check_ids(n, out_regular_key=rk)
        if flags.dtype != torch.uint8 or tuple(flags.shape) != (n,):
            raise ValueError("out_flags must be (n,) torch.uint8")
        for t in (account_id, flags, rk):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device entry point needs contiguous CUDA tensors")
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        N.check(N.load().stl_acctdir_lookup_device(self._h, p(account_id), n, p(flags), p(rk), _stream_ptr(stream)),
                "stl_acctdir_lookup_device")
        return {"flags": flags, "regular_key": rk}

    def tx_blob_authority_device(self, blobs, offsets, lengths, signer_ids=True, accounts=True, stream=None,
                                 out_signer_id=None, out_account=None, out_authority=None):
        """stl_acctdir_tx_blob_authority_device: serialized transactions in HBM
        (as tx_blob_signer_batch_device takes them) -> dict of signer_id
        (n, 20) or None, account (n, 20) or None, and authority (n,) of AUTH_*."""
        import torch
        n = offsets.shape[0]
        dev = blobs.device
        signer = out_signer_id if out_signer_id is not None else (
            torch.empty((n, ACCOUNT_ID_BYTES), dtype=torch.uint8, device=dev) if signer_ids else None)
        account = out_account if out_account is not None else (
            torch.empty((n, ACCOUNT_ID_BYTES), dtype=torch.uint8, device=dev) if accounts else None)
        authority = torch.empty((n,), dtype=torch.uint8, device=dev) if out_authority is None else out_authority
        _check_ids(n, out_signer_id=signer, out_account=account)
        if authority.dtype != torch.uint8 or tuple(authority.shape) != (n,):
            raise ValueError("out_authority must be (n,) torch.uint8")
        if blobs.dtype != torch.uint8:
            raise ValueError("blobs must be torch.uint8")
        _check_rows(blobs, offsets, lengths, signer, account, authority)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        N.check(N.load().stl_acctdir_tx_blob_authority_device(
            self._h, p(blobs), p(offsets), p(lengths), n, p(signer), p(account), p(authority), _stream_ptr(stream)),
            "stl_acctdir_tx_blob_authority_device")
        return {"signer_id": signer, "account": account, "authority": authority}

    def tx_blob_authority(self, blobs, signer_ids=True, accounts=True):
        """stl_acctdir_tx_blob_authority: checkSig's verdict for each
        serialized transaction (list of bytes).  Returns (signer_id (n, 20) or
        None, account (n, 20) or None, authority uint8[n])."""
        n = len(blobs)
        buf, offs, lens = _pack(blobs)
        signer = np.zeros((max(n, 1), ACCOUNT_ID_BYTES), dtype=np.uint8) if signer_ids else None
        account = np.zeros((max(n, 1), ACCOUNT_ID_BYTES), dtype=np.uint8) if accounts else None
        authority = np.zeros(max(n, 1), dtype=np.uint8)
        N.check(N.load().stl_acctdir_tx_blob_authority(
            self._h, _buf(buf), _buf(offs), _buf(lens), n, _buf(signer) if signer_ids else None,
            _buf(account) if accounts else None, _buf(authority)), "stl_acctdir_tx_blob_authority")
        return (signer[:n] if signer_ids else None), (account[:n] if accounts else None), authority[:n]


# ---- verified-ID cache (stl_sigcache_*) ----

SIGCACHE_MAX_SETS_LOG2, SIGCACHE_WAYS = N.STL_SIGCACHE_MAX_SETS_LOG2, N.STL_SIGCACHE_WAYS


class SigCacheInfo(ctypes.Structure):
    """stl_sigcache_info (include/stl.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("sets_log2", ctypes.c_uint32), ("ways", ctypes.c_uint32),
                ("kind", ctypes.c_uint32), ("predicate", ctypes.c_uint32), ("device", ctypes.c_int32),
                ("bytes", ctypes.c_uint64), ("seed", ctypes.c_uint64)]


class SigCache(_DeviceObject):
    """A device-resident cache of the IDs of signed objects the verify has
    accepted (stl_sigcache_create), bound to one blob kind and one accept
    predicate (``policy``: the policy bit, N.STL_DEBUG_RAW_PREDICATE).  A row
    whose ID is found skips the Ed25519 verify; the outputs are those of
    signed_blob_verify_batch_device on every input.

        with SigCache(20) as c:
            out = c.signed_blob_verify_batch_device(blobs, offsets, lengths)   # ingest
            out = c.signed_blob_verify_batch_device(blobs, offsets, lengths)   # ledger close: all hits
    """

    _prefix, _Info = "stl_sigcache", SigCacheInfo

    def __init__(self, sets_log2, kind=BLOB_TRANSACTION, policy=POLICY_SODIUM_1_0_18, seed=0):
        h = ctypes.c_void_p()
        N.check(N.load().stl_sigcache_create(int(sets_log2), int(kind), int(policy), int(seed), ctypes.byref(h)),
                "stl_sigcache_create")
        self._h = h

    def clear(self, stream=None):
        """Empties the cache: a memset enqueued on ``stream``."""
        N.check(N.load().stl_sigcache_clear(self._h, _stream_ptr(stream)), "stl_sigcache_clear")

    def lookup_device(self, ids, out_words=None, stream=None):
        """ids (n, 32) uint8 CUDA tensor -> int64[ceil(n/64)] bitmap words, bit
        i = ID i is present (async on ``stream``)."""
        import torch
        if ids.dtype != torch.uint8:
            raise ValueError("ids must be torch.uint8")
        if ids.dim() != 2 or ids.shape[1] != 32:
            raise ValueError("ids must be (n, 32) bytes")
        n = ids.shape[0]
        if out_words is None:
            out_words = torch.empty((n + 63) // 64, dtype=torch.int64, device=ids.device)
        if out_words.dtype != torch.int64 or out_words.numel() < (n + 63) // 64:
            raise ValueError("out_words must be int64, one word per 64 rows")
        for t in (ids, out_words):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device entry point needs contiguous CUDA tensors")
        N.check(N.load().stl_sigcache_lookup_device(self._h, ctypes.c_void_p(ids.data_ptr()), n,
                                                    ctypes.c_void_p(out_words.data_ptr()), _stream_ptr(stream)),
                "stl_sigcache_lookup_device")
        return out_words

    def signed_blob_verify_batch_device(self, blobs, offsets, lengths, out_words=None, tx_ids=False, flags=None,
                                        stream=None, out_status=None, out_ids=None):
        """Serialized transactions / validations (the cache's kind) in HBM ->
        dict of words, status, tx_id (as verify.signed_blob_verify_batch_device
        writes them), hits and verified.  ``flags``: the cache's predicate by
        default; execution flags (FULL_LENGTH, ...) may be ORed to it.  Waits
        once on ``stream`` (for the probe)."""
        import torch
        n = offsets.shape[0]
        dev = blobs.device
        if out_words is None:
            out_words = torch.empty(((n + 63) // 64,), dtype=torch.int64, device=dev)
        status = torch.empty((n,), dtype=torch.uint8, device=dev) if out_status is None else out_status
        tx_id = out_ids if out_ids is not None else (torch.empty((n, 32), dtype=torch.uint8, device=dev)
                                                     if tx_ids else None)
        if status.dtype != torch.uint8 or (tx_id is not None and tx_id.dtype != torch.uint8):
            raise ValueError("out_status / out_ids must be torch.uint8")
        if tx_id is not None and tx_id.dim() > 1 and tx_id.shape[-1] != 32:
            raise ValueError("out_ids must be (n, 32) bytes")
        if status.numel() < n or (tx_id is not None and tx_id.numel() < 32 * n):
            raise ValueError("status / id buffers smaller than the batch")
        if out_words.dtype != torch.int64 or out_words.numel() < (n + 63) // 64:
            raise ValueError("out_words must be int64, one word per 64 rows")
        if blobs.dtype != torch.uint8:
            raise ValueError("blobs must be torch.uint8")
        _check_rows(blobs, offsets, lengths, out_words, status, tx_id)
        if flags is None:
            flags = self.info()["predicate"]
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        hits, verified = ctypes.c_size_t(0), ctypes.c_size_t(0)
        N.check(N.load().stl_sigcache_signed_blob_verify_batch_device(
            self._h, p(blobs), p(offsets), p(lengths), n, p(out_words), p(status), p(tx_id), int(flags),
            _stream_ptr(stream), ctypes.byref(hits), ctypes.byref(verified)),
            "stl_sigcache_signed_blob_verify_batch_device")
        return {"words": out_words, "status": status, "tx_id": tx_id, "hits": int(hits.value),
                "verified": int(verified.value)}

    def signed_blob_verify_batch(self, blobs, ids=False, flags=None):
        """Host form: list of bytes -> (accept bool[n], status uint8[n], ids
        (n, 32) or None, hits, verified)."""
        n = len(blobs)
        buf, offs, lens = _pack(blobs)
        bitmap = np.zeros((n + 7) // 8 or 1, dtype=np.uint8)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        idb = np.zeros((max(n, 1), 32), dtype=np.uint8) if ids else None
        if flags is None:
            flags = self.info()["predicate"]
        hits, verified = ctypes.c_size_t(0), ctypes.c_size_t(0)
        N.check(N.load().stl_sigcache_signed_blob_verify_batch(
            self._h, _buf(buf), _buf(offs), _buf(lens), n, _buf(bitmap), _buf(status), _buf(idb) if ids else None,
            int(flags), ctypes.byref(hits), ctypes.byref(verified)), "stl_sigcache_signed_blob_verify_batch")
        return (unpack_bitmap(bitmap, n), status[:n], idb[:n] if ids else None, int(hits.value),
                int(verified.value))


# ---- SHAMap root (stl_shamap_root*) ----

SHAMAP_MAX_ITEMS = N.STL_SHAMAP_MAX_ITEMS


def _check_hashes(n, **ts):
    """Keys, leaf hashes and the root are raw bytes: uint8, (n, 32)."""
    import torch
    for name, t in ts.items():
        if t is None:
            continue
        if t.dtype != torch.uint8:
            raise ValueError(f"{name} must be torch.uint8")
        if tuple(t.shape) != (n, 32):
            raise ValueError(f"{name} must be ({1 if name == 'out_root' else 'n'}, 32) bytes")


def shamap_root_device(keys, leaf_hashes=None, select_words=None, out_root=None, counts=False, stream=None):
    """stl_shamap_root_device: the SHAMap root of the set of keys (n, 32) uint8
    in HBM -> (1, 32) uint8 root, or (root, int32[4] counts) with ``counts``
    (True, or a tensor to write them to: distinct items, duplicates dropped,
    inner nodes, deepest depth).  leaf_hashes (n, 32) or None (the leaf hash is
    the key: a transaction set); select_words int64[ceil(n/64)] or None (every
    row), the accept bitmaps' layout.  Asynchronous on ``stream``, no host
    wait.  A deferred row's ID from a blob call is zero: clear its select bit
    or supply its ID."""
    import torch
    if keys.dim() != 2:
        raise ValueError("keys must be (n, 32) bytes")
    n = keys.shape[0]
    _check_hashes(n, keys=keys, leaf_hashes=leaf_hashes)
    if n > SHAMAP_MAX_ITEMS:
        raise ValueError("more than SHAMAP_MAX_ITEMS rows")
    if select_words is not None and (select_words.dtype != torch.int64 or select_words.numel() < (n + 63) // 64):
        raise ValueError("select_words must be int64, one word per 64 rows")
    if out_root is None:
        out_root = torch.empty((1, 32), dtype=torch.uint8, device=keys.device)
    _check_hashes(1, out_root=out_root)
    cnt = None
    if counts is True:
        cnt = torch.empty(4, dtype=torch.int32, device=keys.device)
    elif counts is not False and counts is not None:
        cnt = counts
        if cnt.dtype != torch.int32 or tuple(cnt.shape) != (4,):
            raise ValueError("counts must be int32[4]")
    for t in (keys, leaf_hashes, select_words, out_root, cnt):
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise ValueError("device entry point needs contiguous CUDA tensors")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    N.check(N.load().stl_shamap_root_device(p(keys), p(leaf_hashes), p(select_words), n, p(out_root), p(cnt),
                                            _stream_ptr(stream)), "stl_shamap_root_device")
    return out_root if cnt is None else (out_root, cnt)


def shamap_root(keys, leaf_hashes=None, select=None, counts=False):
    """stl_shamap_root: host memory, synchronous.  keys (n, 32) uint8;
    leaf_hashes (n, 32) or None; select: bool[n] or None -> 32 root bytes, or
    (root, [4 counts]) with ``counts``."""
    keys = np.ascontiguousarray(keys)
    if keys.dtype != np.uint8 or keys.ndim != 2 or keys.shape[1] != 32:
        raise ValueError("keys must be (n, 32) uint8")
    n = keys.shape[0]
    if leaf_hashes is not None:
        leaf_hashes = np.ascontiguousarray(leaf_hashes)
        if leaf_hashes.dtype != np.uint8 or leaf_hashes.shape != (n, 32):
            raise ValueError("leaf_hashes must be (n, 32) uint8")
    sel = None
    if select is not None:
        select = np.asarray(select)
        if select.dtype != np.bool_ or select.shape != (n,):
            raise ValueError("select must be bool[n]")
        sel = np.packbits(select, bitorder="little") if n else np.zeros(1, np.uint8)
    if n > SHAMAP_MAX_ITEMS:
        raise ValueError("more than SHAMAP_MAX_ITEMS rows")
    root = np.zeros(32, dtype=np.uint8)
    cnt = np.zeros(4, dtype=np.uint32)
    N.check(N.load().stl_shamap_root(_buf(keys) if n else None, _buf(leaf_hashes) if leaf_hashes is not None and n
                                     else None, _buf(sel) if sel is not None else None, n, _buf(root), _buf(cnt)),
            "stl_shamap_root")
    return (root.tobytes(), [int(x) for x in cnt]) if counts else root.tobytes()


# ---- resident SHAMap (stl_shamap_tree_*) ----

class ShamapTreeInfo(ctypes.Structure):
    """stl_shamap_tree_info (include/stl.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("capacity", ctypes.c_uint32), ("items", ctypes.c_uint32),
                ("bucket_depth", ctypes.c_uint32), ("device", ctypes.c_int32), ("bytes", ctypes.c_uint64),
                ("root", ctypes.c_uint8 * 32)]


class ShamapTree(_DeviceObject):
    """A device-resident SHAMap (stl_shamap_tree_create): the tree's keys and
    leaf hashes stay in HBM, ``apply_device`` merges a batch of changes (set or
    delete per row; of equal keys the last row counts) and gives the new root,
    rehashing only the buckets the batch touches.

        with ShamapTree(capacity) as t:
            t.apply_device(keys, leaf_hashes)                 # load
            root = t.apply_device(changed, new_hashes, ops)   # each ledger
    """

    _prefix, _Info = "stl_shamap_tree", ShamapTreeInfo

    def __init__(self, capacity):
        h = ctypes.c_void_p()
        N.check(N.load().stl_shamap_tree_create(int(capacity), ctypes.byref(h)), "stl_shamap_tree_create")
        self._h = h

    def info(self):
        """Waits for the device: capacity, exact items, bucket_depth, device,
        bytes, root (32 bytes)."""
        i = super().info()
        i["root"] = bytes(i["root"])
        return i

    # What the apply and the fork wrappers share: `name` the entry point,
    # `handles` the tree handles it takes first.
    def _batch_device(self, name, handles, keys, leaf_hashes, ops, out_root, cnt, nodes, stream):
        import torch
        if keys is None:  # a fork of no rows
            keys = torch.empty((0, 32), dtype=torch.uint8, device="cuda")
        if keys.dim() != 2:
            raise ValueError("keys must be (n, 32) bytes")
        n = keys.shape[0]
        _check_hashes(n, keys=keys, leaf_hashes=leaf_hashes)
        if ops is not None and (ops.dtype != torch.uint8 or tuple(ops.shape) != (n,)):
            raise ValueError("ops must be uint8[n]")
        if out_root is None:
            out_root = torch.empty((1, 32), dtype=torch.uint8, device=keys.device)
        _check_hashes(1, out_root=out_root)
        if nodes is not None:
            cnt = _node_counts(cnt, 8, keys.device)
            nodes = _device_nodes(nodes[0], nodes[1], nodes[2], nodes[3], keys.device)
        elif cnt is True:
            cnt = torch.empty(8, dtype=torch.int32, device=keys.device)
        elif cnt is False or cnt is None:
            cnt = None
        elif cnt.dtype != torch.int32 or tuple(cnt.shape) != (8,):
            raise ValueError("counts must be int32[8]")
        for t in (keys, leaf_hashes, ops, out_root, cnt):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device entry point needs contiguous CUDA tensors")
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        args = [*handles, p(keys), p(leaf_hashes), p(ops), n, p(out_root), p(cnt)]
        if nodes is not None:
            out = nodes.struct()
            args.append(ctypes.byref(out))
        N.check(getattr(N.load(), name)(*args, _stream_ptr(stream)), name)
        return out_root, cnt, nodes

    def _batch_host(self, name, handles, keys, leaf_hashes, ops, nodes):
        if keys is None:  # a fork of no rows
            keys = np.zeros((0, 32), np.uint8)
        keys = np.ascontiguousarray(keys)
        if keys.dtype != np.uint8 or keys.ndim != 2 or keys.shape[1] != 32:
            raise ValueError("keys must be (n, 32) uint8")
        n = keys.shape[0]
        if leaf_hashes is not None:
            leaf_hashes = np.ascontiguousarray(leaf_hashes)
            if leaf_hashes.dtype != np.uint8 or leaf_hashes.shape != (n, 32):
                raise ValueError("leaf_hashes must be (n, 32) uint8")
        if ops is not None:
            ops = np.ascontiguousarray(ops)
            if ops.dtype not in (np.uint8, np.bool_) or ops.shape != (n,):
                raise ValueError("ops must be uint8[n] or bool[n]")
            ops = ops.astype(np.uint8)
        root = np.zeros(32, dtype=np.uint8)
        cnt = np.zeros(8, dtype=np.uint32)
        args = [*handles, _buf(keys) if n else None, _buf(leaf_hashes) if leaf_hashes is not None and n else None,
                _buf(ops) if ops is not None and n else None, n, _buf(root), _buf(cnt)]
        if nodes is not None:
            nodes = HostNodes(*nodes)
            out = nodes.struct()
            args.append(ctypes.byref(out))
        N.check(getattr(N.load(), name)(*args), name)
        return root.tobytes(), [int(x) for x in cnt], nodes

    def apply_device(self, keys, leaf_hashes=None, ops=None, out_root=None, counts=False, stream=None):
        """stl_shamap_tree_apply_device: keys (n, 32) uint8 in HBM, leaf_hashes
        (n, 32) or None (the leaf hash is the key), ops uint8[n] (0 set, else
        delete) or None (all sets) -> (1, 32) uint8 root, or (root, int32[8]
        counts) with ``counts`` (True, or a tensor to write them to).
        Asynchronous on ``stream``."""
        if keys is None:
            raise ValueError("keys must be (n, 32) bytes")
        root, cnt, _ = self._batch_device("stl_shamap_tree_apply_device", [self._h], keys, leaf_hashes, ops, out_root,
                                          counts, None, stream)
        return root if cnt is None else (root, cnt)

    def apply(self, keys, leaf_hashes=None, ops=None, counts=False):
        """stl_shamap_tree_apply: host memory, synchronous.  keys (n, 32) uint8,
        leaf_hashes (n, 32) or None, ops uint8[n] or bool[n] or None -> 32 root
        bytes, or (root, [8 counts]) with ``counts``."""
        if keys is None:
            raise ValueError("keys must be (n, 32) uint8")
        root, cnt, _ = self._batch_host("stl_shamap_tree_apply", [self._h], keys, leaf_hashes, ops, None)
        return (root, cnt) if counts else root

    def root_device(self, out_root=None, stream=None):
        """The current root -> (1, 32) uint8 CUDA tensor (async on ``stream``)."""
        import torch
        if out_root is None:
            out_root = torch.empty((1, 32), dtype=torch.uint8, device="cuda")
        _check_hashes(1, out_root=out_root)
        if not out_root.is_cuda or not out_root.is_contiguous():
            raise ValueError("device entry point needs contiguous CUDA tensors")
        N.check(N.load().stl_shamap_tree_root_device(self._h, ctypes.c_void_p(out_root.data_ptr()),
                                                     _stream_ptr(stream)), "stl_shamap_tree_root_device")
        return out_root

    def export_device(self, out_keys, out_leaf_hashes=None, out_items=None, stream=None):
        """The sorted content -> out_keys / out_leaf_hashes ((rows, 32) uint8
        CUDA tensors, rows at least the host's bound of the count: the capacity
        always serves) and out_items (int32[1], made when None).  Returns
        out_items; async on ``stream``."""
        import torch
        if out_keys.dim() != 2:
            raise ValueError("out_keys must be (n, 32) bytes")
        rows = out_keys.shape[0]
        _check_hashes(rows, out_keys=out_keys, out_leaf_hashes=out_leaf_hashes)
        if out_items is None:
            out_items = torch.zeros(1, dtype=torch.int32, device=out_keys.device)
        if out_items.dtype != torch.int32 or out_items.numel() != 1:
            raise ValueError("out_items must be int32[1]")
        for t in (out_keys, out_leaf_hashes, out_items):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device entry point needs contiguous CUDA tensors")
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        N.check(N.load().stl_shamap_tree_export_device(self._h, p(out_keys), p(out_leaf_hashes), rows, p(out_items),
                                                       _stream_ptr(stream)), "stl_shamap_tree_export_device")
        return out_items


    def apply_nodes_device(self, keys, leaf_hashes=None, ops=None, max_nodes=None, nodes=None, ids=True, meta=True,
                           out_root=None, counts=True, stream=None):
        """stl_shamap_tree_apply_nodes_device: ``apply_device``, and the new
        tree's inner nodes of the dirty buckets and of the prefixes above them
        -> (root, counts, nodes); ``nodes`` as ``shamap_nodes_device`` gives
        it.  Asynchronous on ``stream``."""
        if keys is None:
            raise ValueError("keys must be (n, 32) bytes")
        return self._batch_device("stl_shamap_tree_apply_nodes_device", [self._h], keys, leaf_hashes, ops, out_root,
                                  counts, (nodes, max_nodes, ids, meta), stream)

    def apply_nodes(self, keys, leaf_hashes=None, ops=None, max_nodes=0, ids=True, meta=True):
        """stl_shamap_tree_apply_nodes: host memory, synchronous -> (32 root
        bytes, [8 counts], nodes); ``nodes`` as ``shamap_nodes`` gives it."""
        if keys is None:
            raise ValueError("keys must be (n, 32) uint8")
        return self._batch_host("stl_shamap_tree_apply_nodes", [self._h], keys, leaf_hashes, ops,
                                (max_nodes, ids, meta))

    # ---- SHAMap::snapShot: a fork into another handle, and the one-step revert ----
    def _fork_handles(self, dst):
        if not isinstance(dst, ShamapTree):
            raise ValueError("dst must be a ShamapTree")
        if dst is self:
            raise ValueError("a tree cannot be forked into itself")
        return [self._h, dst._h]

    def fork_device(self, dst, keys=None, leaf_hashes=None, ops=None, out_root=None, counts=False, stream=None):
        """stl_shamap_tree_fork_device: ``dst`` becomes this tree's content with
        the batch applied (``apply_device``'s arguments and results); this tree
        is only read.  ``keys`` None: the plain snapshot.  Asynchronous on
        ``stream``."""
        root, cnt, _ = self._batch_device("stl_shamap_tree_fork_device", self._fork_handles(dst), keys, leaf_hashes,
                                          ops, out_root, counts, None, stream)
        return root if cnt is None else (root, cnt)

    def fork(self, dst, keys=None, leaf_hashes=None, ops=None, counts=False):
        """stl_shamap_tree_fork: host memory, synchronous; as ``apply``."""
        root, cnt, _ = self._batch_host("stl_shamap_tree_fork", self._fork_handles(dst), keys, leaf_hashes, ops, None)
        return (root, cnt) if counts else root

    def fork_nodes_device(self, dst, keys=None, leaf_hashes=None, ops=None, max_nodes=None, nodes=None, ids=True,
                          meta=True, out_root=None, counts=True, stream=None):
        """stl_shamap_tree_fork_nodes_device: ``fork_device``, and the inner
        nodes of ``dst``'s new tree that this tree does not have -> (root,
        counts, nodes), as ``apply_nodes_device``."""
        return self._batch_device("stl_shamap_tree_fork_nodes_device", self._fork_handles(dst), keys, leaf_hashes,
                                  ops, out_root, counts, (nodes, max_nodes, ids, meta), stream)

    def fork_nodes(self, dst, keys=None, leaf_hashes=None, ops=None, max_nodes=0, ids=True, meta=True):
        """stl_shamap_tree_fork_nodes: host memory, synchronous -> (32 root
        bytes, [8 counts], nodes), as ``apply_nodes``."""
        return self._batch_host("stl_shamap_tree_fork_nodes", self._fork_handles(dst), keys, leaf_hashes, ops,
                                (max_nodes, ids, meta))

    def revert(self):
        """stl_shamap_tree_revert: back to what the tree was before the last
        successful apply or fork into it; one step, no device work.  Raises
        where the C call gives STL_EINVAL (nothing to turn back to)."""
        N.check(N.load().stl_shamap_tree_revert(self._h), "stl_shamap_tree_revert")

    def lookup_device(self, keys, out_words=None, leaf_hashes=False, positions=False, stream=None):
        """stl_shamap_tree_lookup_device: keys (n, 32) uint8 in HBM -> found
        words int64[ceil(n/64)] (the accept bitmaps' layout), or (words,
        leaf_hashes, positions) when either is asked for: ``leaf_hashes`` /
        ``positions`` True (made here), a tensor to write ((n, 32) uint8: zeros
        for an absent key; int32[n]: the row in ``export_device``'s order or
        -1), or False (not written, None).  Asynchronous on ``stream``."""
        import torch
        if keys.dim() != 2:
            raise ValueError("keys must be (n, 32) bytes")
        n = keys.shape[0]
        _check_hashes(n, keys=keys)
        if out_words is None:
            out_words = torch.empty(((n + 63) // 64,), dtype=torch.int64, device=keys.device)
        if out_words.dtype != torch.int64 or out_words.numel() < (n + 63) // 64:
            raise ValueError("out_words must be int64, one word per 64 rows")
        leaf = torch.empty((n, 32), dtype=torch.uint8, device=keys.device) if leaf_hashes is True else (
            None if leaf_hashes is False or leaf_hashes is None else leaf_hashes)
        _check_hashes(n, leaf_hashes=leaf)
        pos = torch.empty(n, dtype=torch.int32, device=keys.device) if positions is True else (
            None if positions is False or positions is None else positions)
        if pos is not None and (pos.dtype != torch.int32 or tuple(pos.shape) != (n,)):
            raise ValueError("positions must be int32[n]")
        for t in (keys, out_words, leaf, pos):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device entry point needs contiguous CUDA tensors")
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        N.check(N.load().stl_shamap_tree_lookup_device(self._h, p(keys), n, p(out_words), p(leaf), p(pos),
                                                       _stream_ptr(stream)), "stl_shamap_tree_lookup_device")
        return out_words if leaf is None and pos is None else (out_words, leaf, pos)

    def lookup(self, keys, leaf_hashes=False, positions=False):
        """stl_shamap_tree_lookup: host memory, synchronous.  keys (n, 32)
        uint8 -> found bool[n], or (found, leaf hashes (n, 32) or None,
        positions uint32[n] or None) when either is asked for."""
        keys = np.ascontiguousarray(keys)
        if keys.dtype != np.uint8 or keys.ndim != 2 or keys.shape[1] != 32:
            raise ValueError("keys must be (n, 32) uint8")
        n = keys.shape[0]
        bitmap = np.zeros((n + 7) // 8 or 1, dtype=np.uint8)
        leaf = np.zeros((max(n, 1), 32), np.uint8) if leaf_hashes else None
        pos = np.zeros(max(n, 1), np.uint32) if positions else None
        N.check(N.load().stl_shamap_tree_lookup(self._h, _buf(keys) if n else None, n, _buf(bitmap),
                                                _buf(leaf) if leaf is not None else None,
                                                _buf(pos) if pos is not None else None), "stl_shamap_tree_lookup")
        found = unpack_bitmap(bitmap, n)
        if not leaf_hashes and not positions:
            return found
        return found, leaf[:n] if leaf is not None else None, pos[:n] if pos is not None else None

    def compare_device(self, other, max_rows=None, diff=None, leaf_a=True, leaf_b=True, stream=None):
        """stl_shamap_tree_compare_device: the differences of this tree (a) and
        ``other`` (b) -> a DeviceDiff: rows in key order, the first ``max_rows``
        of them, and int32[8] counts.  Asynchronous on ``stream``."""
        if not isinstance(other, ShamapTree):
            raise ValueError("other must be a ShamapTree")
        if diff is None:
            if max_rows is None:
                raise ValueError("give max_rows (rows to make room for) or diff (a DeviceDiff)")
            diff = DeviceDiff(max_rows, leaf_a, leaf_b)
        elif not isinstance(diff, DeviceDiff):
            raise ValueError("diff must be a DeviceDiff")
        out = diff.struct()
        N.check(N.load().stl_shamap_tree_compare_device(self._h, other._h, ctypes.byref(out), _stream_ptr(stream)),
                "stl_shamap_tree_compare_device")
        return diff

    def compare(self, other, max_rows=0, leaf_a=True, leaf_b=True):
        """stl_shamap_tree_compare: host memory, synchronous -> a HostDiff
        whose arrays hold ``rows()`` rows."""
        if not isinstance(other, ShamapTree):
            raise ValueError("other must be a ShamapTree")
        diff = HostDiff(max_rows, leaf_a, leaf_b)
        out = diff.struct()
        N.check(N.load().stl_shamap_tree_compare(self._h, other._h, ctypes.byref(out)), "stl_shamap_tree_compare")
        return diff

    # ---- SHAMap::getFetchPack: this tree's inner nodes that another tree does not hold ----
    @staticmethod
    def _have_handle(have):
        if have is None:
            return None
        if not isinstance(have, ShamapTree):
            raise ValueError("have must be a ShamapTree or None")
        return have._h

    def fetch_pack_device(self, have=None, max_nodes=None, nodes=None, ids=True, meta=True, counts=False,
                          stream=None):
        """stl_shamap_tree_fetch_pack_device: every inner node of this tree
        (want) for which ``have`` holds no inner node at the same ID with the
        same hash -> a ``DeviceNodes`` of ``max_nodes`` rows (made here, or the
        one given as ``nodes``), or (nodes, int32[8] counts) with ``counts``
        (True, or a tensor to write them to).  ``have`` None: every inner node
        of this tree.  Both trees are only read.  The leaves of the pack are
        ``compare_device(have)``'s A_ONLY and CHANGED rows.  Asynchronous on
        ``stream``."""
        hh = self._have_handle(have)
        nodes = _device_nodes(nodes, max_nodes, ids, meta, "cuda")
        cnt = _node_counts(counts, 8, nodes.count.device)
        if cnt is not None and (not cnt.is_cuda or not cnt.is_contiguous()):
            raise ValueError("device entry point needs contiguous CUDA tensors")
        out = nodes.struct()
        N.check(N.load().stl_shamap_tree_fetch_pack_device(
            self._h, hh, ctypes.byref(out), ctypes.c_void_p(cnt.data_ptr()) if cnt is not None else None,
            _stream_ptr(stream)), "stl_shamap_tree_fetch_pack_device")
        return nodes if cnt is None else (nodes, cnt)

    def fetch_pack(self, have=None, max_nodes=0, ids=True, meta=True):
        """stl_shamap_tree_fetch_pack: host memory, synchronous -> (nodes,
        [8 counts]): a ``HostNodes`` whose arrays hold min(count, max_nodes)
        rows."""
        hh = self._have_handle(have)
        nodes = HostNodes(max_nodes, ids, meta)
        cnt = np.zeros(8, dtype=np.uint32)
        out = nodes.struct()
        N.check(N.load().stl_shamap_tree_fetch_pack(self._h, hh, ctypes.byref(out), _buf(cnt)),
                "stl_shamap_tree_fetch_pack")
        return nodes, [int(x) for x in cnt]

    # ---- SHAMap::getNodeFat / getPath: nodes by node ID, paths by key ----
    def get_nodes_device(self, ids, depths, modes=None, max_nodes=None, nodes=None, node_ids=True, meta=True,
                         leaves=True, counts=False, stream=None):
        """stl_shamap_tree_get_nodes_device: n requests (ids (n, 32) uint8,
        depths uint8[n], modes uint8[n] of SHAMAP_GET_* or None: every request
        FAT) -> a ``GetAnswer``: status uint8[n] (SHAMAP_AT_*), first / rows
        int32[n] (request i's rows are nodes rows first[i] .. first[i] +
        rows[i]), leaf_key / leaf_hash (n, 32) uint8 or None (``leaves``
        False), nodes (a ``DeviceNodes`` of ``max_nodes`` rows, made here, or
        the one given), counts int32[8] or None.  The tree is only read.
        Asynchronous on ``stream``."""
        import torch
        if ids is None or ids.dim() != 2:
            raise ValueError("ids must be (n, 32) bytes")
        n = ids.shape[0]
        _check_hashes(n, ids=ids)
        if n > SHAMAP_GET_MAX_REQUESTS:
            raise ValueError("more than SHAMAP_GET_MAX_REQUESTS requests")
        for name, t in (("depths", depths), ("modes", modes)):
            if t is None and name == "modes":
                continue
            if t is None or t.dtype != torch.uint8 or tuple(t.shape) != (n,):
                raise ValueError(f"{name} must be uint8[n]")
        nodes = _device_nodes(nodes, max_nodes, node_ids, meta, "cuda")
        dev = nodes.count.device
        cnt = _node_counts(counts, 8, dev)
        rows = max(n, 1)  # a place to point at even for no request
        a = GetAnswer()
        a.n, a.nodes, a.counts = n, nodes, cnt
        a.status = torch.empty(rows, dtype=torch.uint8, device=dev)
        a.first = torch.empty(rows, dtype=torch.int32, device=dev)
        a.rows = torch.empty(rows, dtype=torch.int32, device=dev)
        a.leaf_key = torch.empty((rows, 32), dtype=torch.uint8, device=dev) if leaves else None
        a.leaf_hash = torch.empty((rows, 32), dtype=torch.uint8, device=dev) if leaves else None
        for t in (ids, depths, modes, cnt):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device entry point needs contiguous CUDA tensors")
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        out = nodes.struct()
        N.check(N.load().stl_shamap_tree_get_nodes_device(
            self._h, p(ids), p(depths), p(modes), n, p(a.status), p(a.first), p(a.rows), p(a.leaf_key),
            p(a.leaf_hash), ctypes.byref(out), p(cnt), _stream_ptr(stream)), "stl_shamap_tree_get_nodes_device")
        return a

    def get_nodes(self, ids, depths, modes=None, max_nodes=0, node_ids=True, meta=True, leaves=True):
        """stl_shamap_tree_get_nodes: host memory, synchronous.  ids (n, 32)
        uint8, depths uint8[n], modes uint8[n] or None -> a ``GetAnswer`` of
        numpy arrays: nodes a ``HostNodes`` whose arrays hold min(count,
        max_nodes) rows, counts a list of 8 ints."""
        ids = np.ascontiguousarray(ids)
        if ids.dtype != np.uint8 or ids.ndim != 2 or ids.shape[1] != 32:
            raise ValueError("ids must be (n, 32) uint8")
        n = ids.shape[0]
        if n > SHAMAP_GET_MAX_REQUESTS:
            raise ValueError("more than SHAMAP_GET_MAX_REQUESTS requests")
        depths = np.ascontiguousarray(depths)
        if depths.dtype != np.uint8 or depths.shape != (n,):
            raise ValueError("depths must be uint8[n]")
        if modes is not None:
            modes = np.ascontiguousarray(modes)
            if modes.dtype != np.uint8 or modes.shape != (n,):
                raise ValueError("modes must be uint8[n]")
        a = GetAnswer()
        a.n, a.nodes = n, HostNodes(max_nodes, node_ids, meta)
        rows = max(n, 1)
        a.status = np.zeros(rows, np.uint8)
        a.first, a.rows = np.zeros(rows, np.uint32), np.zeros(rows, np.uint32)
        a.leaf_key = np.zeros((rows, 32), np.uint8) if leaves else None
        a.leaf_hash = np.zeros((rows, 32), np.uint8) if leaves else None
        cnt = np.zeros(8, dtype=np.uint32)
        out = a.nodes.struct()
        b = lambda x: _buf(x) if x is not None and n else None  # noqa: E731
        N.check(N.load().stl_shamap_tree_get_nodes(
            self._h, b(ids), b(depths), b(modes), n, _buf(a.status), _buf(a.first), _buf(a.rows),
            _buf(a.leaf_key) if leaves else None, _buf(a.leaf_hash) if leaves else None, ctypes.byref(out),
            _buf(cnt)), "stl_shamap_tree_get_nodes")
        a.counts = [int(x) for x in cnt]
        return a


SHAMAP_GET_MAX_REQUESTS = N.STL_SHAMAP_GET_MAX_REQUESTS
SHAMAP_GET_NODE, SHAMAP_GET_FAT, SHAMAP_GET_PATH = N.STL_SHAMAP_GET_NODE, N.STL_SHAMAP_GET_FAT, N.STL_SHAMAP_GET_PATH
SHAMAP_AT_ABSENT, SHAMAP_AT_INNER, SHAMAP_AT_LEAF = N.STL_SHAMAP_AT_ABSENT, N.STL_SHAMAP_AT_INNER, N.STL_SHAMAP_AT_LEAF
SHAMAP_AT_EMPTY_ROOT, SHAMAP_AT_INVALID = N.STL_SHAMAP_AT_EMPTY_ROOT, N.STL_SHAMAP_AT_INVALID
SHAMAP_AT_OTHER_LEAF = N.STL_SHAMAP_AT_OTHER_LEAF


class GetAnswer:
    """What ``ShamapTree.get_nodes[_device]`` returns: n, status, first, rows,
    leaf_key, leaf_hash, nodes (DeviceNodes / HostNodes) and counts; the first
    ``n`` entries of the per-request arrays are the answers."""

    def request_rows(self, i):
        """(first, rows) of request i as ints (waits for the device)."""
        return int(self.first[i]), int(self.rows[i])


# ---- the difference of two resident trees (stl_shamap_tree_compare*) ----

SHAMAP_DIFF_A_ONLY = N.STL_SHAMAP_DIFF_A_ONLY
SHAMAP_DIFF_B_ONLY = N.STL_SHAMAP_DIFF_B_ONLY
SHAMAP_DIFF_CHANGED = N.STL_SHAMAP_DIFF_CHANGED


def _diff_struct(max_rows, key, kind, leaf_a, leaf_b, counts):
    p = lambda a: a if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731
    return N.ShamapDiffOut(ctypes.sizeof(N.ShamapDiffOut), max_rows, p(key), p(kind), p(leaf_a), p(leaf_b), p(counts))


class DeviceDiff:
    """The rows a device compare writes, as CUDA tensors of ``max_rows`` rows:
    key (max_rows, 32) uint8, kind uint8[max_rows] (SHAMAP_DIFF_*), leaf_a /
    leaf_b (max_rows, 32) uint8 or None, counts int32[8] -- [0] the
    differences, which may exceed max_rows.  Tensors given are written in place."""

    def __init__(self, max_rows, leaf_a=True, leaf_b=True, device="cuda", key=None, kind=None, counts=None):
        import torch
        self.max_rows = int(max_rows)
        if not 0 <= self.max_rows <= SHAMAP_MAX_NODES:
            raise ValueError("max_rows must be in 0 .. SHAMAP_MAX_NODES")
        rows = max(self.max_rows, 1)  # a place to point at even for no row
        u8 = lambda: torch.empty((rows, 32), dtype=torch.uint8, device=device)  # noqa: E731
        self.key = u8() if key is None else key
        self.kind = torch.empty(rows, dtype=torch.uint8, device=device) if kind is None else kind
        self.leaf_a = u8() if leaf_a is True else (None if leaf_a is False or leaf_a is None else leaf_a)
        self.leaf_b = u8() if leaf_b is True else (None if leaf_b is False or leaf_b is None else leaf_b)
        self.counts = torch.zeros(8, dtype=torch.int32, device=device) if counts is None else counts
        for name, t, dt, width in (("key", self.key, torch.uint8, 32), ("kind", self.kind, torch.uint8, None),
                                   ("leaf_a", self.leaf_a, torch.uint8, 32), ("leaf_b", self.leaf_b, torch.uint8, 32),
                                   ("counts", self.counts, torch.int32, None)):
            if t is None:
                continue
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"diff.{name} must be a contiguous CUDA tensor of {dt}")
            need = 8 if name == "counts" else self.max_rows
            if (t.dim() != 2 or t.shape[1] != width or t.shape[0] < need) if width else t.numel() < need:
                raise ValueError(f"diff.{name} has no room for {'8 counts' if name == 'counts' else 'max_rows rows'}")

    def struct(self):
        return _diff_struct(self.max_rows, self.key, self.kind, self.leaf_a, self.leaf_b, self.counts)

    def rows(self):
        """Waits for the device: the rows written, min(counts[0], max_rows)."""
        return min(int(self.counts[0].item()), self.max_rows)


class HostDiff:
    """The same in host memory (numpy), filled by the host form: ``counts`` is
    a list of 8 ints once the call has returned."""

    def __init__(self, max_rows, leaf_a=True, leaf_b=True):
        self.max_rows = int(max_rows)
        if not 0 <= self.max_rows <= SHAMAP_MAX_NODES:
            raise ValueError("max_rows must be in 0 .. SHAMAP_MAX_NODES")
        rows = max(self.max_rows, 1)
        self.key = np.zeros((rows, 32), np.uint8)
        self.kind = np.zeros(rows, np.uint8)
        self.leaf_a = np.zeros((rows, 32), np.uint8) if leaf_a else None
        self.leaf_b = np.zeros((rows, 32), np.uint8) if leaf_b else None
        self._counts = np.zeros(8, np.uint32)

    def struct(self):
        return _diff_struct(self.max_rows, self.key, self.kind, self.leaf_a, self.leaf_b, self._counts)

    @property
    def counts(self):
        return [int(x) for x in self._counts]

    def rows(self):
        return min(int(self._counts[0]), self.max_rows)


# ---- SHAMap inner nodes (stl_shamap_nodes*, stl_shamap_tree_apply_nodes*) ----

SHAMAP_MAX_NODES = N.STL_SHAMAP_MAX_NODES
SHAMAP_NODE_BODY_BYTES = N.STL_SHAMAP_NODE_BODY_BYTES


def _nodes_struct(max_nodes, hash_, body, ids, meta, count):
    p = lambda a: a if a is None or isinstance(a, int) else (  # noqa: E731
        a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
    return N.ShamapNodesOut(ctypes.sizeof(N.ShamapNodesOut), max_nodes, p(hash_), p(body), p(ids), p(meta), p(count))


class DeviceNodes:
    """The inner nodes a device call stores, as CUDA tensors of ``max_nodes``
    rows: hash (max_nodes, 32) uint8, body (max_nodes, 512) uint8, ids
    (max_nodes, 32) uint8 or None, meta int32[max_nodes] or None, count
    int32[1] -- the nodes the call produced, which may exceed max_nodes; rows
    in no particular order.  Tensors given are written in place."""

    def __init__(self, max_nodes, ids=True, meta=True, device="cuda", hash=None, body=None, count=None):  # noqa: A002
        import torch
        self.max_nodes = int(max_nodes)
        if not 0 <= self.max_nodes <= SHAMAP_MAX_NODES:
            raise ValueError("max_nodes must be in 0 .. SHAMAP_MAX_NODES")
        rows = max(self.max_nodes, 1)  # a place to point at even for no row
        u8 = lambda w: torch.empty((rows, w), dtype=torch.uint8, device=device)  # noqa: E731
        self.hash = u8(32) if hash is None else hash
        self.body = u8(512) if body is None else body
        self.ids = u8(32) if ids is True else (None if ids is False else ids)
        self.meta = torch.empty(rows, dtype=torch.int32, device=device) if meta is True else (
            None if meta is False else meta)
        self.count = torch.zeros(1, dtype=torch.int32, device=device) if count is None else count
        for name, t, dt, width in (("hash", self.hash, torch.uint8, 32), ("body", self.body, torch.uint8, 512),
                                   ("ids", self.ids, torch.uint8, 32), ("meta", self.meta, torch.int32, None),
                                   ("count", self.count, torch.int32, None)):
            if t is None:
                continue
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"nodes.{name} must be a contiguous CUDA tensor of {dt}")
            need = 1 if name == "count" else self.max_nodes
            if (t.dim() != 2 or t.shape[1] != width or t.shape[0] < need) if width else t.numel() < need:
                raise ValueError(f"nodes.{name} has no room for max_nodes rows")

    def struct(self):
        return _nodes_struct(self.max_nodes, self.hash, self.body, self.ids, self.meta, self.count)

    def rows(self):
        """Waits for the device: the rows written, min(count, max_nodes)."""
        return min(int(self.count.item()), self.max_nodes)


class HostNodes:
    """The same in host memory (numpy), filled by a host form: ``count`` is an
    int once the call has returned, and the arrays hold ``rows()`` rows."""

    def __init__(self, max_nodes, ids=True, meta=True):
        self.max_nodes = int(max_nodes)
        if not 0 <= self.max_nodes <= SHAMAP_MAX_NODES:
            raise ValueError("max_nodes must be in 0 .. SHAMAP_MAX_NODES")
        rows = max(self.max_nodes, 1)
        self.hash = np.zeros((rows, 32), np.uint8)
        self.body = np.zeros((rows, 512), np.uint8)
        self.ids = np.zeros((rows, 32), np.uint8) if ids else None
        self.meta = np.zeros(rows, np.uint32) if meta else None
        self._count = np.zeros(1, np.uint32)

    def struct(self):
        return _nodes_struct(self.max_nodes, self.hash, self.body, self.ids, self.meta, self._count)

    @property
    def count(self):
        return int(self._count[0])

    def rows(self):
        return min(self.count, self.max_nodes)


def _node_counts(counts, words, device):
    import torch
    if counts is True:
        return torch.empty(words, dtype=torch.int32, device=device)
    if counts is False or counts is None:
        return None
    if counts.dtype != torch.int32 or tuple(counts.shape) != (words,):
        raise ValueError(f"counts must be int32[{words}]")
    return counts


def _device_nodes(nodes, max_nodes, ids, meta, device):
    if nodes is not None:
        if not isinstance(nodes, DeviceNodes):
            raise ValueError("nodes must be a DeviceNodes")
        return nodes
    if max_nodes is None:
        raise ValueError("give max_nodes (rows to make room for) or nodes (a DeviceNodes)")
    return DeviceNodes(max_nodes, ids, meta, device)


def shamap_nodes_device(keys, leaf_hashes=None, select_words=None, max_nodes=None, nodes=None, ids=True, meta=True,
                        out_root=None, counts=True, stream=None):
    """stl_shamap_nodes_device: ``shamap_root_device``, and every inner node of
    the map stored once -> (root, counts, nodes): root (1, 32) uint8, counts
    int32[4] (or None with ``counts=False``), nodes a ``DeviceNodes`` of
    ``max_nodes`` rows (made here, or the one given).  A map of m keys has at
    most 63 (m - 1) + 1 inner nodes; when nodes.count exceeds max_nodes the
    arrays hold some max_nodes of them and root and counts are still right.
    Asynchronous on ``stream``, no host wait."""
    import torch
    if keys.dim() != 2:
        raise ValueError("keys must be (n, 32) bytes")
    n = keys.shape[0]
    _check_hashes(n, keys=keys, leaf_hashes=leaf_hashes)
    if n > SHAMAP_MAX_ITEMS:
        raise ValueError("more than SHAMAP_MAX_ITEMS rows")
    if select_words is not None and (select_words.dtype != torch.int64 or select_words.numel() < (n + 63) // 64):
        raise ValueError("select_words must be int64, one word per 64 rows")
    if out_root is None:
        out_root = torch.empty((1, 32), dtype=torch.uint8, device=keys.device)
    _check_hashes(1, out_root=out_root)
    cnt = _node_counts(counts, 4, keys.device)
    nodes = _device_nodes(nodes, max_nodes, ids, meta, keys.device)
    for t in (keys, leaf_hashes, select_words, out_root, cnt):
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise ValueError("device entry point needs contiguous CUDA tensors")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    out = nodes.struct()
    N.check(N.load().stl_shamap_nodes_device(p(keys), p(leaf_hashes), p(select_words), n, p(out_root), p(cnt),
                                             ctypes.byref(out), _stream_ptr(stream)), "stl_shamap_nodes_device")
    return out_root, cnt, nodes


def shamap_nodes(keys, leaf_hashes=None, select=None, max_nodes=0, ids=True, meta=True):
    """stl_shamap_nodes: host memory, synchronous -> (32 root bytes, [4
    counts], nodes): a ``HostNodes`` whose arrays hold min(count, max_nodes)
    rows."""
    keys = np.ascontiguousarray(keys)
    if keys.dtype != np.uint8 or keys.ndim != 2 or keys.shape[1] != 32:
        raise ValueError("keys must be (n, 32) uint8")
    n = keys.shape[0]
    if leaf_hashes is not None:
        leaf_hashes = np.ascontiguousarray(leaf_hashes)
        if leaf_hashes.dtype != np.uint8 or leaf_hashes.shape != (n, 32):
            raise ValueError("leaf_hashes must be (n, 32) uint8")
    sel = None
    if select is not None:
        select = np.asarray(select)
        if select.dtype != np.bool_ or select.shape != (n,):
            raise ValueError("select must be bool[n]")
        sel = np.packbits(select, bitorder="little") if n else np.zeros(1, np.uint8)
    if n > SHAMAP_MAX_ITEMS:
        raise ValueError("more than SHAMAP_MAX_ITEMS rows")
    root = np.zeros(32, dtype=np.uint8)
    cnt = np.zeros(4, dtype=np.uint32)
    nodes = HostNodes(max_nodes, ids, meta)
    out = nodes.struct()
    N.check(N.load().stl_shamap_nodes(_buf(keys) if n else None, _buf(leaf_hashes) if leaf_hashes is not None and n
                                      else None, _buf(sel) if sel is not None else None, n, _buf(root), _buf(cnt),
                                      ctypes.byref(out)), "stl_shamap_nodes")
    return root.tobytes(), [int(x) for x in cnt], nodes


# ---- registered signer sets (stl_keyset_*) ----

class KeysetInfo(ctypes.Structure):
    """stl_keyset_info (include/stl.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("nkeys", ctypes.c_uint32), ("window_bits", ctypes.c_uint32),
                ("windows", ctypes.c_uint32), ("rows_per_window", ctypes.c_uint32), ("row_bytes", ctypes.c_uint32),
                ("device", ctypes.c_int32), ("reserved", ctypes.c_uint32), ("table_bytes", ctypes.c_uint64)]


class Keyset(_DeviceObject):
    """A registered signer set (stl_keyset_create): per-key comb tables on the
    current device, verified against by key index -- 64 table additions per
    signature, no doubling, the same bits as the per-signature calls.

        with Keyset(pks) as ks:
            words = ks.verify_batch_device(key_index, sig, msg)
    """

    _prefix, _Info = "stl_keyset", KeysetInfo
    _info_skip = ("struct_size", "reserved")

    def __init__(self, pks):
        pks = np.ascontiguousarray(pks, dtype=np.uint8).reshape(-1, 32)
        h = ctypes.c_void_p()
        N.check(N.load().stl_keyset_create(_buf(pks), pks.shape[0], 0, ctypes.byref(h)), "stl_keyset_create")
        self._h = h

    def find(self, pk):
        """First index of the 32-byte key, or -1."""
        pk = bytes(pk)
        if len(pk) != 32:
            raise ValueError("a key is 32 bytes")
        return int(N.load().stl_keyset_find(self._h, pk))

    def verify_batch(self, key_index, sig, msg, policy=POLICY_SODIUM_1_0_18):
        """Host arrays -> bool[n]; an index >= nkeys raises StlError(STL_EINVAL)."""
        key_index = np.ascontiguousarray(key_index, dtype=np.uint32).reshape(-1)
        sig = np.ascontiguousarray(sig, dtype=np.uint8).reshape(-1, 64)
        msg = np.ascontiguousarray(msg, dtype=np.uint8).reshape(-1, 32)
        n = sig.shape[0]
        if msg.shape[0] != n or key_index.shape[0] != n:
            raise ValueError("key_index/sig/msg batch sizes differ")
        bitmap = np.zeros((n + 7) // 8, dtype=np.uint8)
        N.check(N.load().stl_keyset_verify_batch(self._h, _buf(key_index), _buf(sig), _buf(msg), n, _buf(bitmap),
                                                 policy), "stl_keyset_verify_batch")
        return unpack_bitmap(bitmap, n)

    @staticmethod
    def _device_rows(key_index, *ts):
        import torch
        for t in (key_index,) + ts:
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device entry point needs contiguous CUDA tensors")
        if key_index.dtype != torch.int32:
            raise ValueError("key_index must be int32 (the bits of a uint32 index)")

    def verify_batch_device(self, key_index, sig, msg, out_words=None, policy=POLICY_SODIUM_1_0_18, stream=None):
        """key_index (n,) int32 / sig (n,64) / msg (n,32) CUDA tensors -> int64
        bitmap words (async on ``stream``); a row whose index is >= nkeys gets
        bit 0."""
        import torch
        n = sig.shape[0]
        if out_words is None:
            out_words = torch.empty((n + 63) // 64, dtype=torch.int64, device=sig.device)
        self._device_rows(key_index, sig, msg, out_words)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        N.check(N.load().stl_keyset_verify_batch_device(self._h, p(key_index), p(sig), p(msg), n, p(out_words), policy,
                                                        _stream_ptr(stream)), "stl_keyset_verify_batch_device")
        return out_words

    def tx_verify_batch_device(self, key_index, preimages, offsets, lengths, sig, out_words=None,
                               policy=POLICY_SODIUM_1_0_18, stream=None):
        """checkSign / validation form: SHA512Half of each preimage, then the
        keyset verify (same bits as tx_hash_batch_device + verify_batch_device)."""
        import torch
        n = offsets.shape[0]
        if out_words is None:
            out_words = torch.empty(((n + 63) // 64,), dtype=torch.int64, device=preimages.device)
        self._device_rows(key_index, sig, out_words)
        _check_rows(preimages, offsets, lengths)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        N.check(N.load().stl_keyset_tx_verify_batch_device(
            self._h, p(key_index), p(preimages), p(offsets), p(lengths), p(sig), n, p(out_words), policy,
            _stream_ptr(stream)), "stl_keyset_tx_verify_batch_device")
        return out_words

    # ---- by public key: the set need not be closed ----

    @staticmethod
    def _device_keys(*ts):
        import torch
        for t in ts:
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device entry point needs contiguous CUDA tensors")
        for t in ts[:3]:
            if t is not None and t.dtype != torch.uint8:
                raise ValueError("pk / sig / msg must be uint8")

    def lookup_device(self, pk, out_index=None, miss_count=None, stream=None):
        """pk (n,32) uint8 CUDA tensor -> int32[n] key indices (the bits of
        uint32; N.STL_KEYSET_NOT_FOUND, i.e. -1, for a key that is not in the
        set), async on ``stream``.  ``miss_count``: an int32 CUDA tensor whose
        first element receives the number of rows not found."""
        import torch
        n = pk.shape[0]
        if out_index is None:
            out_index = torch.empty(n, dtype=torch.int32, device=pk.device)
        self._device_keys(pk, None, None, out_index, miss_count)
        if out_index.dtype != torch.int32 or out_index.numel() < n:
            raise ValueError("out_index must be int32, one element per row")
        if miss_count is not None and (miss_count.dtype != torch.int32 or miss_count.numel() < 1):
            raise ValueError("miss_count must be an int32 tensor")
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        N.check(N.load().stl_keyset_lookup_device(self._h, p(pk), n, p(out_index), p(miss_count),
                                                  _stream_ptr(stream)), "stl_keyset_lookup_device")
        return out_index

    def verify_by_key_device(self, pk, sig, msg, out_words=None, policy=POLICY_SODIUM_1_0_18, stream=None):
        """pk (n,32) / sig (n,64) / msg (n,32) CUDA tensors -> (int64 bitmap
        words, misses): the bits of verify_batch_device(sig, msg, pk);
        registered signers from the tables, the ``misses`` other rows through
        the per-signature kernels.  Waits once on ``stream`` (for the lookup);
        the words are complete when ``stream`` reaches the call's end."""
        import torch
        n = sig.shape[0]
        if out_words is None:
            out_words = torch.empty((n + 63) // 64, dtype=torch.int64, device=sig.device)
        self._device_keys(pk, sig, msg, out_words)
        if pk.shape[0] != n or msg.shape[0] != n:
            raise ValueError("pk/sig/msg batch sizes differ")
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        misses = ctypes.c_size_t(0)
        N.check(N.load().stl_keyset_verify_by_key_device(self._h, p(pk), p(sig), p(msg), n, p(out_words), policy,
                                                         _stream_ptr(stream), ctypes.byref(misses)),
                "stl_keyset_verify_by_key_device")
        return out_words, int(misses.value)

    def verify_by_key(self, pk, sig, msg, policy=POLICY_SODIUM_1_0_18):
        """Host arrays -> bool[n] (the bits of verify_batch(sig, msg, pk))."""
        pk = np.ascontiguousarray(pk, dtype=np.uint8).reshape(-1, 32)
        sig = np.ascontiguousarray(sig, dtype=np.uint8).reshape(-1, 64)
        msg = np.ascontiguousarray(msg, dtype=np.uint8).reshape(-1, 32)
        n = sig.shape[0]
        if msg.shape[0] != n or pk.shape[0] != n:
            raise ValueError("pk/sig/msg batch sizes differ")
        bitmap = np.zeros((n + 7) // 8, dtype=np.uint8)
        N.check(N.load().stl_keyset_verify_by_key(self._h, _buf(pk), _buf(sig), _buf(msg), n, _buf(bitmap), policy),
                "stl_keyset_verify_by_key")
        return unpack_bitmap(bitmap, n)

    def signed_blob_verify_batch_device(self, blobs, offsets, lengths, out_words=None, tx_ids=False,
                                        policy=POLICY_SODIUM_1_0_18, stream=None, kind=None, out_status=None,
                                        out_ids=None):
        """Serialized validations / transactions in HBM, verified by each
        row's SigningPubKey against the set -> dict of words, status, tx_id (as
        verify.signed_blob_verify_batch_device) and misses."""
        import torch
        n = offsets.shape[0]
        dev = blobs.device
        if out_words is None:
            out_words = torch.empty(((n + 63) // 64,), dtype=torch.int64, device=dev)
        status = torch.empty((n,), dtype=torch.uint8, device=dev) if out_status is None else out_status
        tx_id = out_ids if out_ids is not None else (torch.empty((n, 32), dtype=torch.uint8, device=dev)
                                                     if tx_ids else None)
        if status.dtype != torch.uint8 or (tx_id is not None and tx_id.dtype != torch.uint8):
            raise ValueError("out_status / out_ids must be torch.uint8")
        if tx_id is not None and tx_id.dim() > 1 and tx_id.shape[-1] != 32:
            raise ValueError("out_ids must be (n, 32) bytes")
        if status.numel() < n or (tx_id is not None and tx_id.numel() < 32 * n):
            raise ValueError("status / id buffers smaller than the batch")
        _check_rows(blobs, offsets, lengths, out_words, status, tx_id)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        misses = ctypes.c_size_t(0)
        N.check(N.load().stl_keyset_signed_blob_verify_batch_device(
            self._h, N.STL_BLOB_TRANSACTION if kind is None else kind, p(blobs), p(offsets), p(lengths), n,
            p(out_words), p(status), p(tx_id), policy, _stream_ptr(stream), ctypes.byref(misses)),
            "stl_keyset_signed_blob_verify_batch_device")
        return {"words": out_words, "status": status, "tx_id": tx_id, "misses": int(misses.value)}

    def rows(self, key, first_row, nrows):
        """Test hook (stl_debug_keyset_rows): table rows of key ``key``
        (N.STL_KEYSET_BASE: the base point's) -> uint32[nrows, row_bytes / 4]."""
        words = self.info()["row_bytes"] // 4
        out = np.zeros((nrows, words), dtype=np.uint32)
        N.check(N.load().stl_debug_keyset_rows(self._h, key, first_row, nrows, _buf(out)), "stl_debug_keyset_rows")
        return out


class Batcher:
    """stl_batcher (include/stl.h): single requests from any thread, run as
    device batches by max_batch / max_delay_us; ``submit`` / ``submit_tx``
    return a Future-like handle whose ``result()`` is the verdict
    (VERDICT_ACCEPT / VERDICT_REJECT / VERDICT_DEFER or a negative STL_E*)."""

    class Handle:
        def __init__(self):
            import threading
            self._ev = threading.Event()
            self.verdict = None

        def result(self, timeout=None):
            if not self._ev.wait(timeout):
                raise TimeoutError("verdict not delivered")
            return self.verdict

    def __init__(self, max_batch=4096, max_delay_us=1000, policy=POLICY_SODIUM_1_0_18):
        import threading
        self._lib = N.load()
        self._b = self._lib.stl_batcher_create(max_batch, max_delay_us, policy)
        if not self._b:
            raise ValueError("stl_batcher_create rejected its arguments")
        self._live = {}
        self._mu = threading.Lock()
        self._next = 0

        def done(ctx, verdict):
            with self._mu:
                h = self._live.pop(ctx)
            h.verdict = verdict
            h._ev.set()

        self._cb = N.VERDICT_FN(done)  # kept alive with the aggregator

    def _register(self):
        h = Batcher.Handle()
        with self._mu:
            self._next += 1
            key = self._next
            self._live[key] = h
        return key, h

    def submit(self, sig, msg32, pk):
        key, h = self._register()
        N.check(self._lib.stl_batcher_submit(self._b, bytes(sig), bytes(msg32), bytes(pk), self._cb, key),
                "stl_batcher_submit")
        return h

    def submit_tx(self, blob):
        key, h = self._register()
        blob = bytes(blob)
        N.check(self._lib.stl_batcher_submit_tx(self._b, blob, len(blob), self._cb, key), "stl_batcher_submit_tx")
        return h

    def flush(self):
        self._lib.stl_batcher_flush(self._b)

    def stats(self):
        v = [ctypes.c_uint64(0) for _ in range(3)]
        self._lib.stl_batcher_stats(self._b, *[ctypes.byref(x) for x in v])
        return {"submitted": v[0].value, "completed": v[1].value, "batches": v[2].value}

    def close(self):
        if self._b:
            self._lib.stl_batcher_destroy(self._b)
            self._b = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


VERDICT_REJECT, VERDICT_ACCEPT, VERDICT_DEFER = N.STL_VERDICT_REJECT, N.STL_VERDICT_ACCEPT, N.STL_VERDICT_DEFER


# ---- one process per GPU: the RCCL bitmap gather (include/stl.h) ----

def comm_unique_id():
    """stl_comm_unique_id: 128 bytes for rank 0 to hand to every rank."""
    buf = ctypes.create_string_buffer(128)
    N.check(N.load().stl_comm_unique_id(buf), "stl_comm_unique_id")
    return buf.raw


def comm_init_rank(nranks, rank, uid):
    uid = bytes(uid)
    if len(uid) != 128:
        raise ValueError("unique id is 128 bytes")
    N.check(N.load().stl_comm_init_rank(nranks, rank, uid), "stl_comm_init_rank")


def comm_destroy():
    N.load().stl_comm_destroy()


def comm_abort():
    """stl_comm_abort: tear the communicator down without waiting for peers."""
    N.load().stl_comm_abort()


def comm_sync(stream=None, timeout_ms=0):
    """stl_comm_sync: wait for ``stream`` under the RCCL deadline; raises
    StlError (STL_ERCCL) after aborting the communicator if a gather stalls."""
    N.check(N.load().stl_comm_sync(_stream_ptr(stream), int(timeout_ms)), "stl_comm_sync")


def comm_info():
    """stl_comm_info: (nranks, rank) as RCCL reports them (ncclCommCount /
    ncclCommUserRank) for the communicator libstl gathers over."""
    nr, r = ctypes.c_int(0), ctypes.c_int(0)
    N.check(N.load().stl_comm_info(ctypes.byref(nr), ctypes.byref(r)), "stl_comm_info")
    return nr.value, r.value


def bitmap_gather_device(words, out_words=None, root=0, stream=None):
    """stl_bitmap_gather_device: every rank's int64 bitmap words (CUDA tensor of
    words_per_rank words) into out_words (nranks*words_per_rank) on rank
    ``root`` (root < 0: all ranks)."""
    ptr = ctypes.c_void_p(out_words.data_ptr()) if out_words is not None else None
    N.check(N.load().stl_bitmap_gather_device(ctypes.c_void_p(words.data_ptr()), words.numel(), ptr, root,
                                              _stream_ptr(stream)), "stl_bitmap_gather_device")
    return out_words


def bitmap_gatherv_device(words, word_offsets, out_words=None, root=0, stream=None):
    """stl_bitmap_gatherv_device: rank r's int64 words (word_offsets[r+1] -
    word_offsets[r] of them) into out_words[word_offsets[r]:] on rank
    ``root``; word_offsets has nranks+1 entries, the same on every rank."""
    offs = np.ascontiguousarray(word_offsets, dtype=np.uint64)
    ptr = ctypes.c_void_p(out_words.data_ptr()) if out_words is not None else None
    wptr = ctypes.c_void_p(words.data_ptr()) if words.numel() else None
    N.check(N.load().stl_bitmap_gatherv_device(wptr, words.numel(), ptr, _buf(offs), root, _stream_ptr(stream)),
            "stl_bitmap_gatherv_device")
    return out_words


# ---- statistics (include/stl.h stl_get_stats) ----

class Stats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("batches", ctypes.c_uint64), ("signatures", ctypes.c_uint64), ("errors", ctypes.c_uint64),
                ("host_ns", ctypes.c_uint64), ("gather_ns", ctypes.c_uint64),
                ("accepted", ctypes.c_uint64), ("full_length_lanes", ctypes.c_uint64),
                ("phase_ns", ctypes.c_uint64 * 4), ("phase_chunks", ctypes.c_uint64),
                ("auto_dedup_chunks", ctypes.c_uint64),
                ("key_cache_hits", ctypes.c_uint64), ("key_cache_misses", ctypes.c_uint64)]


# stl_stats.phase_ns: [0] the first phase-1 kernel -- all of phase 1 when it
# runs as one kernel (the default), the SHA-512 + lattice kernel when split;
# [1] the point-decoding kernel when split, the key-dedup kernels; [2] the main
# kernel; [3] the full-length fallback kernel
PHASES = ("phase1", "point", "main", "fallback")


def get_stats():
    """Counters of include/stl.h stl_get_stats; ``phase_ns`` is a dict of the
    summed kernel time per verify phase (zero unless phase timing is on)."""
    st = Stats()
    st.struct_size = ctypes.sizeof(Stats)
    N.check(N.load().stl_get_stats(ctypes.byref(st)), "stl_get_stats")
    out = {name: getattr(st, name) for name, _ in Stats._fields_
           if name not in ("struct_size", "reserved", "phase_ns")}
    out["phase_ns"] = dict(zip(PHASES, list(st.phase_ns)))
    return out


def reset_stats():
    N.load().stl_reset_stats()


def set_phase_timing(on):
    """Per-phase HIP-event timing of the verify launches (stl_set_phase_timing);
    returns the previous setting."""
    return bool(N.load().stl_set_phase_timing(1 if on else 0))


# ---- testing hooks ----

def debug_fault_after(calls):
    """stl_debug_fault_after: the HIP/RCCL call after ``calls`` more fails (one shot)."""
    N.load().stl_debug_fault_after(calls)


def debug_verify_k_device(sig, k, pk, out_words=None, policy=POLICY_SODIUM_1_0_18, stream=None):
    """stl_debug_verify_k_device: verify with given k (n,32) instead of hashing."""
    import torch
    n = sig.shape[0]
    if out_words is None:
        out_words = torch.empty((n + 63) // 64, dtype=torch.int64, device=sig.device)
    N.check(N.load().stl_debug_verify_k_device(
        ctypes.c_void_p(sig.data_ptr()), ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(pk.data_ptr()), n,
        ctypes.c_void_p(out_words.data_ptr()), policy, _stream_ptr(stream)), "stl_debug_verify_k_device")
    return out_words


TUNE_FUSED_PREP, TUNE_MAIN_QUEUE = N.STL_TUNE_FUSED_PREP, N.STL_TUNE_MAIN_QUEUE
TUNE_STREAMS, TUNE_CHUNK_LOG2 = N.STL_TUNE_STREAMS, N.STL_TUNE_CHUNK_LOG2
TUNE_BYTE_SHARDS = N.STL_TUNE_BYTE_SHARDS
TUNE_QUAD = N.STL_TUNE_QUAD
TUNE_STREAM_WORKSPACES = N.STL_TUNE_STREAM_WORKSPACES
TUNE_RCCL_TIMEOUT_MS = N.STL_TUNE_RCCL_TIMEOUT_MS
TUNE_LONG_HASH = N.STL_TUNE_LONG_HASH
TUNE_SHARED_KEYS = N.STL_TUNE_SHARED_KEYS
TUNE_WIDE_MIN_ROWS = N.STL_TUNE_WIDE_MIN_ROWS
TUNE_R_AHEAD = N.STL_TUNE_R_AHEAD
TUNE_FIRST_CHUNK = N.STL_TUNE_FIRST_CHUNK
TUNE_KEY_CACHE = N.STL_TUNE_KEY_CACHE


def debug_tuning(key, value):
    """stl_debug_tuning: process-wide execution setting (same accept bits
    whatever the value); returns the previous value."""
    rc = N.load().stl_debug_tuning(key, value)
    if rc < 0:
        raise N.StlError(rc, "stl_debug_tuning")
    return rc


def release_stream(stream):
    """stl_release_stream: free libstl's context of a caller stream (a torch
    stream) on the current device."""
    N.check(N.load().stl_release_stream(_stream_ptr(stream)), "stl_release_stream")


def stream_contexts():
    """Caller-stream contexts libstl keeps on the current device
    (at most debug_tuning(TUNE_STREAM_WORKSPACES, -1))."""
    rc = N.load().stl_debug_stream_contexts()
    if rc < 0:
        N.check(rc, "stl_debug_stream_contexts")
    return rc


def clock_stamp(nwg=256, stream=None):
    """stl_debug_clock_stamp: (nwg, 4) int64 CUDA tensor of {shader cycle
    counter, 100 MHz counter, XCC_ID, HW_ID} per one-wave workgroup, enqueued
    on ``stream`` (bench.py's clock_ghz)."""
    import torch
    out = torch.zeros((nwg, 4), dtype=torch.int64, device="cuda")
    N.check(N.load().stl_debug_clock_stamp(ctypes.c_void_p(out.data_ptr()), nwg, _stream_ptr(stream)),
            "stl_debug_clock_stamp")
    return out


def selftest_ops_device(op, rows, out=None, stream=None):
    """stl_debug_selftest_ops_device (tests only): ``op`` on ``rows``, an
    (n, STL_SELFTEST_IN_WORDS) int32 CUDA tensor of raw words; returns the
    (n, STL_SELFTEST_OUT_WORDS) int32 results (``out``, if given, receives
    them at its start)."""
    import torch
    n = rows.shape[0]
    if out is None:
        out = torch.empty((n, N.STL_SELFTEST_OUT_WORDS), dtype=torch.int32, device=rows.device)
    N.check(N.load().stl_debug_selftest_ops_device(op, ctypes.c_void_p(rows.data_ptr()), n,
                                                   ctypes.c_void_p(out.data_ptr()), _stream_ptr(stream)),
            "stl_debug_selftest_ops_device")
    return out


def selftest_group_device(op, group, rows, out=None, stream=None):
    """stl_debug_selftest_group_device (tests only): lane-group formula
    ``op`` with ``group`` = 2 or 4 lanes per row; returns (n * group,
    STL_SELFTEST_OUT_WORDS) int32 records, one per lane."""
    import torch
    n = rows.shape[0]
    if out is None:
        out = torch.empty((n * group, N.STL_SELFTEST_OUT_WORDS), dtype=torch.int32, device=rows.device)
    N.check(N.load().stl_debug_selftest_group_device(op, group, ctypes.c_void_p(rows.data_ptr()), n,
                                                     ctypes.c_void_p(out.data_ptr()), _stream_ptr(stream)),
            "stl_debug_selftest_group_device")
    return out


def clock_ghz(start, end):
    """Average shader clock (GHz) between two clock_stamp results (numpy or
    torch (nwg, 4)).  Each CU keeps its own cycle counter (tools/clock_probe.py:
    counters of one XCD differ by ~1e8 cycles at one instant), so stamps are
    matched per CU -- XCC_ID and HW_ID bits 8-15 (CU, SH, SE) -- and the clock
    of each CU is its cycle delta over its 100 MHz delta.  Returns (median over
    the CUs found in both stamps, {xcc: median over its CUs}, CUs matched)."""
    a = start.cpu().numpy() if hasattr(start, "cpu") else np.asarray(start)
    b = end.cpu().numpy() if hasattr(end, "cpu") else np.asarray(end)

    def by_cu(x):
        d = {}
        for t, rt, xcc, hw in x.tolist():
            d.setdefault((int(xcc) & 0xF, (int(hw) >> 8) & 0xFF), []).append((t, rt))
        return {k: (float(np.median([v[0] for v in vs])), float(np.median([v[1] for v in vs])))
                for k, vs in d.items()}
    sa, sb = by_cu(a), by_cu(b)
    per_cu = {}
    for k in sorted(set(sa) & set(sb)):
        dr = sb[k][1] - sa[k][1]
        if dr > 0:
            per_cu[k] = (sb[k][0] - sa[k][0]) / dr * 0.1
    if not per_cu:
        return None, {}, 0
    per_xcc = {}
    for (xcc, _), v in per_cu.items():
        per_xcc.setdefault(xcc, []).append(v)
    vals = sorted(per_cu.values())
    return vals[len(vals) // 2], {x: float(np.median(v)) for x, v in sorted(per_xcc.items())}, len(per_cu)


def execution_settings():
    """The current stl_debug_tuning values."""
    lib = N.load()
    return {name: lib.stl_debug_tuning(key, -1) for name, key in (
        ("fused_prep", TUNE_FUSED_PREP), ("main_queue", TUNE_MAIN_QUEUE), ("streams", TUNE_STREAMS),
        ("chunk_log2", TUNE_CHUNK_LOG2), ("quad", TUNE_QUAD), ("long_hash", TUNE_LONG_HASH),
        ("shared_keys", TUNE_SHARED_KEYS), ("wide_min_rows", TUNE_WIDE_MIN_ROWS),
        ("r_ahead", TUNE_R_AHEAD), ("first_chunk", TUNE_FIRST_CHUNK), ("key_cache", TUNE_KEY_CACHE))}


def key_cache_clear():
    """stl_debug_key_cache_clear: empty the current device's decoded-key cache."""
    N.check(N.load().stl_debug_key_cache_clear(), "stl_debug_key_cache_clear")


def key_cache_info():
    """stl_debug_key_cache_info: {"ptr", "bytes", "sets_log2", "ways"} of the
    current device's decoded-key cache (bytes 0: none)."""
    p, b = ctypes.c_void_p(), ctypes.c_uint64()
    k, w = ctypes.c_uint32(), ctypes.c_uint32()
    N.check(N.load().stl_debug_key_cache_info(ctypes.byref(p), ctypes.byref(b), ctypes.byref(k), ctypes.byref(w)),
            "stl_debug_key_cache_info")
    return {"ptr": p.value or 0, "bytes": b.value, "sets_log2": k.value, "ways": w.value}


def sign_batch_device(seed, msg, stream=None):
    """RFC 8032 keypair(seed) + detached signature over msg, on the GPU.
    seed (n,32), msg (n,32) uint8 CUDA tensors -> (pk (n,32), sig (n,64))."""
    import torch
    n = seed.shape[0]
    pk = torch.empty((n, 32), dtype=torch.uint8, device=seed.device)
    sig = torch.empty((n, 64), dtype=torch.uint8, device=seed.device)
    N.check(N.load().stl_ed25519_sign_batch_device(
        ctypes.c_void_p(seed.data_ptr()), ctypes.c_void_p(msg.data_ptr()), n, ctypes.c_void_p(pk.data_ptr()),
        ctypes.c_void_p(sig.data_ptr()), _stream_ptr(stream)), "stl_ed25519_sign_batch_device")
    return pk, sig


def sign_adversarial_device(seed, msg, cls, param, stream=None):
    """Test data: sign_batch_device, then rows with cls (n,) uint8 in 1..11
    mutated into SURVEY Appendix-B class B<cls> with parameter param (n,)
    int32 (tests/datasets.py).  -> (pk, sig, msg) CUDA tensors."""
    import torch
    n = seed.shape[0]
    pk = torch.empty((n, 32), dtype=torch.uint8, device=seed.device)
    sig = torch.empty((n, 64), dtype=torch.uint8, device=seed.device)
    mo = torch.empty((n, 32), dtype=torch.uint8, device=seed.device)
    for t in (seed, msg, cls, param):
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("device entry point needs contiguous CUDA tensors")
    N.check(N.load().stl_debug_sign_adversarial_device(
        ctypes.c_void_p(seed.data_ptr()), ctypes.c_void_p(msg.data_ptr()), ctypes.c_void_p(cls.data_ptr()),
        ctypes.c_void_p(param.data_ptr()), n, ctypes.c_void_p(pk.data_ptr()), ctypes.c_void_p(sig.data_ptr()),
        ctypes.c_void_p(mo.data_ptr()), _stream_ptr(stream)), "stl_debug_sign_adversarial_device")
    return pk, sig, mo


def words_to_bool(words, n):
    """int64 bitmap words (torch or numpy) -> bool[n] numpy."""
    arr = words.cpu().numpy() if hasattr(words, "cpu") else np.asarray(words)
    return np.unpackbits(arr.astype("<i8").view(np.uint8), bitorder="little")[:n].astype(bool)
