"""The account directory in Python (test infrastructure only): a port of
acctdir_hash (stellard_amd/csrc/stl_acctdir_core.h), a dict model of a
directory, and Transactor::checkSig written from the reference
(Transactor.cpp:151-180; mHasAuthKey at :326, terNO_ACCOUNT at :312-320) --
never from the code under test."""
import ctypes
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCTDIR_SO = os.path.join(ROOT, "tests", "native", "libhostemu_acctdir.so")

HAS_REGULAR_KEY, MASTER_DISABLED, ABSENT, NOT_FOUND = 0x1, 0x2, 0x4, 0xFF
(AUTH_MASTER, AUTH_REGULAR, AUTH_MASTER_DISABLED, AUTH_BAD_AUTH, AUTH_BAD_AUTH_MASTER, AUTH_NO_ACCOUNT,
 AUTH_UNDECIDED) = range(7)

_M64 = (1 << 64) - 1


def _mix(h):
    h ^= h >> 32
    h = (h * 0xff51afd7ed558ccd) & _M64
    h ^= h >> 29
    return h


def acctdir_hash(account_id, seed):
    """acctdir_hash of a 20-byte ID (five little-endian words) under ``seed``."""
    w = struct.unpack("<5I", bytes(account_id))
    c = 0xc4ceb9fe1a85ec53
    h = _mix((seed + 0x9e3779b97f4a7c15) & _M64)
    h = _mix(((h ^ (w[0] | (w[1] << 32))) * c) & _M64)
    h = _mix(((h ^ (w[2] | (w[3] << 32))) * c) & _M64)
    h = _mix(((h ^ (w[4] | (5 << 32))) * c) & _M64)
    h = _mix((h + seed * 0xd6e8feb86659fd93) & _M64)
    return h >> 32


def slots_for(capacity):
    s = 4
    while s < 4 * capacity:
        s <<= 1
    return s


def same_home_ids(count, home, nslots, seed, rng_seed):
    """``count`` distinct random IDs whose home slot in a table of ``nslots``
    slots under ``seed`` is ``home``."""
    rng = np.random.default_rng(rng_seed)
    out = []
    while len(out) < count:
        for row in rng.integers(0, 256, (4096, 20), dtype=np.uint8):
            b = row.tobytes()
            if acctdir_hash(b, seed) & (nslots - 1) == home and b not in out:
                out.append(b)
                if len(out) == count:
                    break
    return out


class Entry:
    """An account root's three fields; regular_key is None without sfRegularKey."""

    def __init__(self, regular_key=None, master_disabled=False):
        self.regular_key = None if regular_key is None else bytes(regular_key)
        self.master_disabled = bool(master_disabled)


def check_sig(signer, account, entry):
    """Transactor::checkSig for a signer ID, the Account and its account root
    (an Entry, or None where there is none)."""
    if entry is None:
        return AUTH_NO_ACCOUNT  # Transactor.cpp:312-320: there is no mTxnAccount to ask
    has_auth_key = entry.regular_key is not None  # :326 isFieldPresent(sfRegularKey)
    if signer == account:  # :155
        if entry.master_disabled:  # :159
            return AUTH_MASTER_DISABLED
        return AUTH_MASTER
    if has_auth_key and signer == entry.regular_key:  # :162
        return AUTH_REGULAR
    if has_auth_key:  # :167
        return AUTH_BAD_AUTH
    return AUTH_BAD_AUTH_MASTER  # :172


class Model:
    """What a directory must answer: ID -> (flags, regular key), every account
    ever upserted (ABSENT ones stay, and still use a record)."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.state = {}

    def upsert(self, ids, flags, keys):
        """True and applied, or False (it does not fit) and unchanged."""
        last = {}
        for i, f, k in zip(ids, flags, keys):
            last[bytes(i)] = (int(f), bytes(k) if int(f) & HAS_REGULAR_KEY else bytes(20))
        if len(self.state) + len(last) > self.capacity:
            return False
        self.state.update(last)
        return True

    def lookup(self, account_id):
        """(flags byte, regular key) as the lookup call reports them."""
        f, k = self.state.get(bytes(account_id), (ABSENT, bytes(20)))
        if f & ABSENT:
            return NOT_FOUND, bytes(20)
        return f, k

    def entry(self, account_id):
        f, k = self.lookup(account_id)
        if f == NOT_FOUND:
            return None
        return Entry(k if f & HAS_REGULAR_KEY else None, bool(f & MASTER_DISABLED))

    def lookup_arrays(self, ids):
        got = [self.lookup(i) for i in ids]
        return (np.array([g[0] for g in got], np.uint8),
                np.frombuffer(b"".join(g[1] for g in got), np.uint8).reshape(-1, 20))


def id_array(ids):
    return np.frombuffer(b"".join(bytes(i) for i in ids), np.uint8).reshape(-1, 20).copy()


def random_batch(rng, known, m):
    """An upsert batch of m rows: fresh IDs, IDs from ``known`` (a list, grown
    here) with new flags and keys, some ABSENT, and duplicates inside the batch."""
    ids, flags, keys = [], [], []
    for _ in range(m):
        r = rng.random()
        if ids and r < 0.15:
            a = ids[int(rng.integers(0, len(ids)))]  # a duplicate inside the batch
        elif known and r < 0.55:
            a = known[int(rng.integers(0, len(known)))]
        else:
            a = rng.bytes(20)
            known.append(a)
        f = int(rng.integers(0, 4))
        if rng.random() < 0.15:
            f |= ABSENT
        ids.append(a)
        flags.append(f)
        keys.append(rng.bytes(20))  # stale bytes where HAS_REGULAR_KEY is not set
    return ids, np.array(flags, np.uint8), keys


def load_acctdir_emu():
    from stellard_amd import build
    build.build_hostemu_acctdir()
    lib = ctypes.CDLL(ACCTDIR_SO)
    V = ctypes.c_void_p
    lib.hostemu_acctdir_slots.restype = ctypes.c_uint32
    lib.hostemu_acctdir_slots.argtypes = [ctypes.c_uint32]
    lib.hostemu_acctdir_hash.restype = ctypes.c_uint32
    lib.hostemu_acctdir_hash.argtypes = [V, ctypes.c_uint64]
    lib.hostemu_acct_authority.restype = ctypes.c_uint32
    lib.hostemu_acct_authority.argtypes = [V, V, ctypes.c_int, ctypes.c_uint32, V]
    lib.hostemu_acctdir_create.restype = V
    lib.hostemu_acctdir_create.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
    lib.hostemu_acctdir_destroy.argtypes = [V]
    lib.hostemu_acctdir_info.argtypes = [V, V]
    lib.hostemu_acctdir_upsert.restype = ctypes.c_int
    lib.hostemu_acctdir_upsert.argtypes = [V, V, V, V, ctypes.c_size_t]
    lib.hostemu_acctdir_lookup.argtypes = [V, V, ctypes.c_size_t, V, V]
    lib.hostemu_acctdir_authority_row.restype = ctypes.c_uint32
    lib.hostemu_acctdir_authority_row.argtypes = [V, V, ctypes.c_uint32, V, V, V]
    return lib


# ---- the authority corpus: signer_cases blobs with directory entries ----
# Each STL_TX_OK row with a 20-byte Account gets one of these, by i mod 8 with
# i the row's number among the rows of its class.
ENTRY_KINDS = ["none", "plain", "master_disabled", "key_signer", "key_random", "absent", "key_signer_disabled",
               "key_account_disabled"]


def corpus_entries(cases, seed):
    """For signer_cases cases: the upsert batch (ids, flags, keys) that gives
    each decided row its entry kind, and each row's expected authority by
    check_sig.  Rows whose Account was already given an entry keep it."""
    rng = np.random.default_rng(seed)
    model = Model(len(cases))
    ids, flags, keys = [], [], []
    seen = {}  # rows so far per class: every class of blob meets every kind of entry
    for c in cases:
        if c.authority == 2:  # signer_cases.UNDECIDED
            continue
        if c.account in model.state:
            continue
        kind = ENTRY_KINDS[seen.get(c.name, 0) % 8]
        seen[c.name] = seen.get(c.name, 0) + 1
        if kind == "none":
            continue
        f, k = 0, rng.bytes(20)
        if kind == "master_disabled":
            f = MASTER_DISABLED
        elif kind == "key_signer":
            f, k = HAS_REGULAR_KEY, c.signer
        elif kind == "key_random":
            f = HAS_REGULAR_KEY
        elif kind == "absent":
            f = ABSENT | int(rng.integers(0, 4))
        elif kind == "key_signer_disabled":
            f, k = HAS_REGULAR_KEY | MASTER_DISABLED, c.signer
        elif kind == "key_account_disabled":
            f, k = HAS_REGULAR_KEY | MASTER_DISABLED, c.account
        ids.append(c.account)
        flags.append(f)
        keys.append(k)
        model.upsert([c.account], [f], [k])
    want = np.array([AUTH_UNDECIDED if c.authority == 2 else check_sig(c.signer, c.account, model.entry(c.account))
                     for c in cases], np.uint8)
    return ids, np.array(flags, np.uint8), keys, want, model
