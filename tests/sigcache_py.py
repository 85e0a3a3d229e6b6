"""The verified-ID cache in Python (test infrastructure only): a port of
sigcache_hash (stellard_amd/csrc/stl_sigcache_core.h), the set and first way
it gives, and a model that knows, for a seed and a list of IDs, which sets
receive more than four distinct IDs -- so a test can say exactly which IDs the
insert guarantee covers."""
import ctypes
import os
import struct
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGCACHE_SO = os.path.join(ROOT, "tests", "native", "libhostemu_sigcache.so")

WAYS = 4
LINE_BYTES = 128
MAX_SETS_LOG2 = 24
PREDICATE_MASK = 0x80000001  # STL_POLICY_MASK | STL_DEBUG_RAW_PREDICATE

_M64 = (1 << 64) - 1


def _mix(h):
    h ^= h >> 32
    h = (h * 0xff51afd7ed558ccd) & _M64
    h ^= h >> 29
    return h


def sigcache_hash(id32, seed):
    """sigcache_hash of a 32-byte ID (eight little-endian words) under ``seed``."""
    w = struct.unpack("<8I", bytes(id32))
    c = 0xc4ceb9fe1a85ec53
    h = _mix((seed + 0x9e3779b97f4a7c15) & _M64)
    for i in range(4):
        h = _mix(((h ^ (w[2 * i] | (w[2 * i + 1] << 32))) * c) & _M64)
    h = _mix(((h ^ (8 << 32)) * c) & _M64)
    h = _mix((h + seed * 0xd6e8feb86659fd93) & _M64)
    return h


def set_of(id32, seed, sets_log2):
    return (sigcache_hash(id32, seed) >> 32) & ((1 << sets_log2) - 1)


def first_way(id32, seed):
    return sigcache_hash(id32, seed) >> 62


def unstorable(id32):
    """An ID whose first 64 bits are zero is never stored and never hits."""
    return bytes(id32)[:8] == bytes(8)


class Model:
    """What a cache of 2^sets_log2 sets under ``seed`` has received since it
    was made or cleared: per set the distinct storable IDs, in arrival order."""

    def __init__(self, sets_log2, seed):
        self.sets_log2, self.seed = sets_log2, seed
        self.sets = {}
        self.last = {}

    def clear(self):
        self.sets.clear()
        self.last.clear()

    def insert(self, ids):
        for i in ids:
            i = bytes(i)
            if unstorable(i):
                continue
            s = set_of(i, self.seed, self.sets_log2)
            self.sets.setdefault(s, OrderedDict())[i] = True
            self.last[s] = i

    def overfull_sets(self):
        """The sets that have received more than WAYS distinct IDs."""
        return {s for s, d in self.sets.items() if len(d) > WAYS}

    def guaranteed(self):
        """The IDs the insert guarantee says are present."""
        return {i for s, d in self.sets.items() if len(d) <= WAYS for i in d}

    def received(self):
        return {i for d in self.sets.values() for i in d}

    def check(self, present):
        """``present``: the set of IDs a lookup of every received ID reported.
        Asserts the guarantee: every ID of a set with at most WAYS arrivals is
        there; of a fuller set at most WAYS are, the last inserted among them."""
        missing = self.guaranteed() - present
        assert not missing, (len(missing), sorted(missing)[:3])
        for s in self.overfull_sets():
            there = [i for i in self.sets[s] if i in present]
            assert len(there) <= WAYS, (s, len(there))
            assert self.last[s] in present, s


def max_set_load(ids, seed, sets_log2):
    """The largest number of distinct storable IDs of ``ids`` that share a set."""
    m = Model(sets_log2, seed)
    m.insert(ids)
    return max((len(d) for d in m.sets.values()), default=0)


def seed_without_overfull_set(ids, sets_log2, first=1):
    """The smallest seed >= ``first`` under which no set receives more than
    WAYS of ``ids``."""
    seed = first
    while max_set_load(ids, seed, sets_log2) > WAYS:
        seed += 1
    return seed


def load_sigcache_emu():
    from stellard_amd import build
    build.build_hostemu_sigcache()  # as every other harness: built on load if absent or stale
    lib = ctypes.CDLL(SIGCACHE_SO)
    P, U8 = ctypes.c_void_p, ctypes.c_void_p
    for name, res, args in (
            ("hostemu_sigcache_hash", ctypes.c_uint64, [U8, ctypes.c_uint64]),
            ("hostemu_sigcache_set", ctypes.c_uint32, [ctypes.c_uint64, ctypes.c_uint32]),
            ("hostemu_sigcache_first_way", ctypes.c_uint32, [ctypes.c_uint64]),
            ("hostemu_sigcache_bytes", ctypes.c_uint64, [ctypes.c_uint32]),
            ("hostemu_sigcache_predicate", ctypes.c_uint32, [ctypes.c_uint32]),
            ("hostemu_sigcache_create", P, [ctypes.c_uint32, ctypes.c_uint64]),
            ("hostemu_sigcache_destroy", None, [P]),
            ("hostemu_sigcache_clear", None, [P]),
            ("hostemu_sigcache_insert", None, [P, U8, ctypes.c_size_t, U8]),
            ("hostemu_sigcache_lookup", None, [P, U8, ctypes.c_size_t, U8]),
            ("hostemu_sigcache_lines", P, [P])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib
