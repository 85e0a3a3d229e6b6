"""Serialized transactions for the signer-authority tests (test infrastructure
only): blobs built with tests/txblob.py whose Account field holds the value
under test, each with the status, signer ID, account and authority the
reference's rules give -- computed here from the fields, never from the code
under test.

  signer ID  Hash160(SigningPubKey) = RippleAddress::getAccountID
             (RippleAddress.cpp:361-363) on every STL_TX_OK row
  authority  MASTER where it equals a 20-byte Account (Transactor.cpp:151-170),
             NOT_MASTER where it does not, UNDECIDED for any other Account
             length and for every row that is not STL_TX_OK (zero IDs)

Signatures and keys are random bytes: nothing here verifies a signature.
"""
import ctypes
import os

import numpy as np

from tests import txblob as T
from tests.hash160_py import hash160

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNER_SO = os.path.join(ROOT, "tests", "native", "libhostemu_signer.so")

NOT_MASTER, MASTER, UNDECIDED = 0, 1, 2
TX_OK, TX_DEFERRED, TX_MALFORMED = 0, 1, 2

CLASSES = ["master", "random_account", "other_key", "first_byte", "last_byte", "account_19", "account_21",
           "account_empty", "deferred", "malformed", "no_account", "extras", "sendmax_invoice", "memos", "paths",
           "memos_paths_master"]


class Case:
    def __init__(self, name, blob, status, signer, account, authority):
        self.name, self.blob, self.status = name, bytes(blob), status
        self.signer, self.account, self.authority = bytes(signer), bytes(account), authority


def _with_account(fields, value):
    out = [f for f in fields if f.fid != T.Account]
    if value is not None:
        out.append(T.Field(T.Account, T.vl(value)))
    return out


def make_case(rng, cls, seq):
    """One blob of class ``cls`` and what the signer pass must say about it."""
    pk, sig = rng.bytes(32), rng.bytes(64)
    me = hash160(pk)
    opts = {}
    if cls == "extras":
        opts = dict(extras=True)
    elif cls in ("memos", "memos_paths_master"):
        opts = dict(memos=int(rng.integers(1, 4)), paths=cls == "memos_paths_master")
    elif cls == "paths":
        opts = dict(paths=True, extras=True)
    fs = T.payment_fields(rng, pk, seq, **opts)
    if cls == "sendmax_invoice":  # both sort ahead of Account and move its offset
        cur, iss = b"\0" * 12 + b"EUR" + b"\0" * 5, rng.bytes(20)
        fs += [T.Field(T.InvoiceID, rng.bytes(32)),
               T.Field(T.SendMax, T.amount_iou(int(rng.integers(10**15, 10**16)), 0, cur, iss))]
    account = me
    if cls in ("random_account", "deferred", "malformed"):
        account = rng.bytes(20)
    elif cls == "other_key":
        account = hash160(rng.bytes(32))
    elif cls == "first_byte":
        account = bytes([me[0] ^ (1 << int(rng.integers(0, 8)))]) + me[1:]
    elif cls == "last_byte":
        account = me[:19] + bytes([me[19] ^ (1 << int(rng.integers(0, 8)))])
    elif cls == "account_19":
        account = me[:19]
    elif cls == "account_21":
        account = me + b"\0"
    elif cls == "account_empty":
        account = b""
    elif cls == "no_account":
        account = None
    elif cls in ("extras", "paths", "memos") and rng.random() < 0.5:
        account = rng.bytes(20)
    fs = _with_account(fs, account)
    status = TX_OK
    if cls == "malformed":  # a 33-byte key: checkSign false, canonical all the same
        fs = [f for f in fs if f.fid != T.SigningPubKey] + [T.Field(T.SigningPubKey, T.vl(pk + b"\0"))]
        status = TX_MALFORMED
    full = sorted(fs + [T.Field(T.TxnSignature, T.vl(sig))], key=lambda f: T.code(f.fid))
    if cls == "deferred":  # two fields out of order
        full[1], full[2] = full[2], full[1]
        status = TX_DEFERRED
    if cls == "no_account":  # SOE_REQUIRED: the reference never constructs it
        status = TX_DEFERRED
    blob = T.serialize(full, sort=False)
    zero = bytes(20)
    if status != TX_OK:
        case = Case(cls, blob, status, zero, zero, UNDECIDED)
    elif account is None or len(account) != 20:
        case = Case(cls, blob, status, me, zero, UNDECIDED)
    else:
        case = Case(cls, blob, status, me, account, MASTER if account == me else NOT_MASTER)
    # where the Account payload lies (header and length byte are one byte each)
    case.acct_off = case.acct_len = None
    if account is not None:
        at = [f.fid for f in full].index(T.Account)
        case.acct_off = len(T.serialize(full[:at], sort=False)) + 2
        case.acct_len = len(account)
    return case


def make_cases(n, seed):
    """n cases, the classes in rotation."""
    rng = np.random.default_rng(seed)
    return [make_case(rng, CLASSES[i % len(CLASSES)], i + 1) for i in range(n)]


def load_signer_emu():
    from stellard_amd import build
    build.build_hostemu_signer()
    lib = ctypes.CDLL(SIGNER_SO)
    V = ctypes.c_void_p
    lib.hostemu_sha256_32.argtypes = [V, V]
    lib.hostemu_ripemd160_32.argtypes = [V, V]
    lib.hostemu_hash160_32.argtypes = [V, ctypes.c_size_t, V]
    lib.hostemu_signer_row.restype = ctypes.c_uint32
    lib.hostemu_signer_row.argtypes = [V, ctypes.c_uint32, V, V, V]
    lib.hostemu_signer_account_pos.argtypes = [V, ctypes.c_uint32, V]
    return lib


def emu_row(lib, blob):
    """(status, signer, account, authority) of the host build's per-row function."""
    b = np.frombuffer(bytes(blob), np.uint8).copy() if len(blob) else np.zeros(1, np.uint8)
    sg, ac = np.zeros(20, np.uint8), np.zeros(20, np.uint8)
    st = ctypes.c_uint32(99)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    auth = lib.hostemu_signer_row(p(b), len(blob), p(sg), p(ac), ctypes.byref(st))
    return st.value, sg.tobytes(), ac.tobytes(), auth


def load_vectors():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "hash160_vectors.json")) as f:
        return json.load(f)
