"""The decoded-key cache's second-choice set and phase 1's split point half on
the host (stellard_amd/csrc/stl_keycache.h and stl_verify_core.h compiled by
tests/native/hostemu_keycache_alt.cpp):

  * the alternate set index is a function of the key alone, differs from the
    primary set under every mask with a set bit and equals it under mask 0,
  * 2^20 random keys inserted one after the other under the insert rule all
    find a place,
  * the insert rule's order over tag-present / empty patterns of both sets,
  * the R half of phase 1 followed by finish_phase1_points gives the state
    verify_phase1_points gives, byte for byte,
  * the crowded-set batch of tests/test_gpu_keycache_fused.py exists.
"""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "native", "libhostemu_keycache_alt.so")
WAYS = 6


class KeyCacheAltEmu:
    def __init__(self):
        from stellard_amd import build
        build.build_hostemu_keycache_alt()
        lib = ctypes.CDLL(SO)
        V, Z, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
        lib.hostemu_kca_bound_violations.restype = ctypes.c_uint64
        lib.hostemu_kca_index.argtypes = [V, Z, U, V, V]
        lib.hostemu_kca_place.argtypes = [Z, V, V, V, V, V, V]
        lib.hostemu_kca_fill.argtypes = [V, Z, U, V]
        lib.hostemu_kca_split.restype = ctypes.c_uint64
        lib.hostemu_kca_split.argtypes = [V, V, V, Z, U, V, V]
        self.lib = lib

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def index(self, keys, mask):
        """-> (primary set uint32[n], alternate set uint32[n]) under `mask`"""
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
        s = np.zeros(keys.shape[0], np.uint32)
        a = np.zeros(keys.shape[0], np.uint32)
        self.lib.hostemu_kca_index(self._p(keys), keys.shape[0], mask, self._p(s), self._p(a))
        return s, a

    def place(self, first, same0, empty0, same1, empty1):
        """-> (way uint32[n], alternate set written bool[n])"""
        arrs = [np.ascontiguousarray(x, np.uint32) for x in (first, same0, empty0, same1, empty1)]
        out = np.zeros(arrs[0].shape[0], np.uint32)
        self.lib.hostemu_kca_place(out.shape[0], *[self._p(x) for x in arrs], self._p(out))
        return out & 7, (out & 8) != 0

    def fill(self, keys, log2_sets):
        """-> (inserts that overwrote another key, keys in their alternate set, keys not found afterwards)"""
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
        out = np.zeros(3, np.uint64)
        self.lib.hostemu_kca_fill(self._p(keys), keys.shape[0], log2_sets, self._p(out))
        return tuple(int(v) for v in out)

    def split(self, sig, msg, pk, policy):
        """-> (rows whose states differ, whole uint8[n, 224], split uint8[n, 224])"""
        sig, msg, pk = (np.ascontiguousarray(x, np.uint8) for x in (sig, msg, pk))
        n = sig.shape[0]
        a, b = np.zeros((n, 224), np.uint8), np.zeros((n, 224), np.uint8)
        d = self.lib.hostemu_kca_split(self._p(sig), self._p(msg), self._p(pk), n, policy, self._p(a), self._p(b))
        return int(d), a, b


@pytest.fixture(scope="module")
def emu():
    return KeyCacheAltEmu()


def test_alternate_index(emu):
    """The cache's masks are 2^K - 1; under each of them from 1 to 2^24 - 1 (and
    under 200 arbitrary masks with a set bit, which the function serves as
    well) the two sets differ for every key and both lie inside the mask."""
    rng = np.random.default_rng(0xA17)
    keys = rng.integers(0, 256, (100000, 32), np.uint8)
    masks = [(1 << k) - 1 for k in range(1, 25)] + [int(m) for m in rng.integers(1, 1 << 24, 200)]
    for mask in masks:
        s, a = emu.index(keys, mask)
        assert (s != a).all(), hex(mask)
        assert not (s & ~np.uint32(mask)).any() and not (a & ~np.uint32(mask)).any(), hex(mask)
    s, a = emu.index(keys, 0)
    assert not s.any() and not a.any()
    # the key alone: the same bytes give the same index wherever they stand,
    # and whatever stands beside them
    mask = (1 << 20) - 1
    s, a = emu.index(keys, mask)
    perm = rng.permutation(keys.shape[0])
    s2, a2 = emu.index(keys[perm], mask)
    assert np.array_equal(a2, a[perm]) and np.array_equal(s2, s[perm])
    one = emu.index(keys[77:78].copy(), mask)[1]
    assert one[0] == a[77]
    # it spreads: of 10^5 keys in 2^20 sets nearly all get an alternate set of their own
    assert np.unique(a).shape[0] > 90000
    # and it does not follow the primary index: keys of one primary set (16 sets) scatter
    s4, a4 = emu.index(keys, 15)
    for p in range(16):
        assert np.unique(a4[s4 == p]).shape[0] == 15


def test_placement_of_2_20_keys(emu):
    """Sequential insertion of 2^20 random keys into the default 2^20 sets:
    every key finds its tag's way or an empty one in one of its two sets."""
    keys = np.random.default_rng(0x0CC).integers(0, 256, (1 << 20, 32), np.uint8)
    evicting, in_alt, lost = emu.fill(keys, 20)
    print("keys placed in their alternate set:", in_alt, "unplaced:", evicting, "not found afterwards:", lost)
    assert evicting == 0 and lost == 0
    assert 0 < in_alt < 1000  # an ideal hash gives 100-120: the keys in primary sets over six


def _rule(first, same0, empty0, same1, empty1):
    """The insert rule, restated: (way, alternate set written)."""
    def lowest(bits):
        return next(w for w in range(WAYS) if bits >> w & 1)

    def nearest(bits):
        return next((first + i) % WAYS for i in range(WAYS) if bits >> ((first + i) % WAYS) & 1)
    if same0:
        return lowest(same0), False
    if empty0:
        return nearest(empty0), False
    if same1:
        return lowest(same1), True
    if empty1:
        return nearest(empty1), True
    return first, False


def test_insert_rule(emu):
    """Every same / empty pattern of the primary set (a way cannot be both)
    against a spread of patterns of the alternate set, for every first way."""
    every = (1 << WAYS) - 1
    prim = [(s, e) for s in range(every + 1) for e in range(every + 1) if not s & e]
    some = sorted({0, every, 0b101010, 0b010101, 0b000110, 0b110000} | {1 << w for w in range(WAYS)})
    alt = [(s, e) for s in some for e in some if not s & e]
    rows = [(f, s0, e0, s1, e1) for f in range(WAYS) for (s0, e0) in prim for (s1, e1) in alt]
    rows += [(f, s1, e1, s0, e0) for f in range(WAYS) for (s0, e0) in prim[::7] for (s1, e1) in alt]
    cols = np.array(rows, np.uint32).T
    way, in_alt = emu.place(*cols)
    exp = [_rule(*r) for r in rows]
    assert np.array_equal(way, np.array([w for w, _ in exp], np.uint32))
    assert np.array_equal(in_alt, np.array([a for _, a in exp], bool))
    # spelled out, for first way 2:
    def one(*r):
        w, a = emu.place(*[[v] for v in r])
        return int(w[0]), bool(a[0])
    assert one(2, 0b001000, 0, 0, every) == (3, False)  # a tag in the primary set wins over an empty alternate way
    assert one(2, 0b001000, 0b000001, 0b000001, 0) == (3, False)  # ... and over an empty primary way
    assert one(2, 0, 0b100001, 0b000100, 0) == (5, False)  # an empty primary way before the tag in the alternate set
    assert one(2, 0, 0, 0b010000, 0b000001) == (4, True)  # the alternate set's tag before its empty way
    assert one(2, 0, 0, 0, 0b000011) == (0, True)  # the nearest empty alternate way counting from the hash's
    assert one(2, 0, 0, 0, 0) == (2, False)  # both full: the primary set's hash way


def test_split_phase1(emu, golden):
    """verify_phase1_points_r, A's decoding and finish_phase1_points against
    verify_phase1_points on the goldens (every adversarial class) and 10,000
    random rows (about a quarter of them with both points decodable), under
    the four core policies: the 224-byte states are equal."""
    rng = np.random.default_rng(0x5B117)
    sig = np.concatenate([golden["sig"], rng.integers(0, 256, (10000, 64), np.uint8)])
    msg = np.concatenate([golden["msg"], rng.integers(0, 256, (10000, 32), np.uint8)])
    pk = np.concatenate([golden["pk"], rng.integers(0, 256, (10000, 32), np.uint8)])
    sig[-10000:, 63] &= 0x0F  # S < L, so the random rows get past the range check
    oks = 0
    for policy in range(4):
        differ, a, b = emu.split(sig, msg, pk, policy)
        assert differ == 0 and np.array_equal(a, b), policy
        oks += int((a[:, 42] & 1).sum())  # kHalfOk: bit 16 of word 10
    assert oks > 1000  # accepted-so-far rows are among them, not only early rejects
    assert emu.lib.hostemu_kca_bound_violations() == 0


CROWDED_SEED = 0xC40D
CROWDED_LOG2 = 10


def crowded_batch(emu):
    """The GPU test's crowded-set batch: from 16,384 signers made of seeded
    random seeds, at 1,024 sets, 8 keys that share one primary set and whose
    alternate sets are pairwise distinct, then the first 56 keys whose two
    sets are none of those nine.  -> (seeds uint8[64, 32], the shared set), or
    None where no such 8 keys exist."""
    from tests import oracle_bind
    n = 16384
    seeds = np.random.default_rng(CROWDED_SEED).integers(0, 256, (n, 32), np.uint8)
    pk, _, _ = oracle_bind.hostemu_sign_adversarial(oracle_bind.load_hostemu(), seeds, np.zeros((n, 32), np.uint8),
                                                    np.zeros(n, np.uint8), np.zeros(n, np.uint32))
    s, a = emu.index(pk, (1 << CROWDED_LOG2) - 1)
    for p in np.argsort(-np.bincount(s, minlength=1 << CROWDED_LOG2), kind="stable"):
        rows = np.flatnonzero(s == p)
        _, first = np.unique(a[rows], return_index=True)  # one key per alternate set
        if first.shape[0] < 8:
            continue
        crowd = rows[np.sort(first)[:8]]
        taken = set(int(v) for v in a[crowd]) | {int(p)}
        rest = [i for i in range(n) if int(s[i]) not in taken and int(a[i]) not in taken][:56]
        if len(rest) == 56:
            return seeds[np.concatenate([crowd, np.array(rest)])], int(p)
    return None


def test_crowded_batch_exists(emu):
    got = crowded_batch(emu)
    assert got is not None
    seeds, p = got
    print("crowded-set batch: seed", hex(CROWDED_SEED), "shared primary set", p)
    from tests import oracle_bind
    pk, _, _ = oracle_bind.hostemu_sign_adversarial(oracle_bind.load_hostemu(), seeds, np.zeros((64, 32), np.uint8),
                                                    np.zeros(64, np.uint8), np.zeros(64, np.uint32))
    assert np.unique(pk, axis=0).shape[0] == 64
    s, a = emu.index(pk, (1 << CROWDED_LOG2) - 1)
    assert (s[:8] == p).all() and np.unique(a[:8]).shape[0] == 8
    nine = set(int(v) for v in a[:8]) | {p}
    assert not any(int(v) in nine for v in s[8:]) and not any(int(v) in nine for v in a[8:])
