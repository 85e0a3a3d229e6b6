"""The decoded-key cache's logic on the host (stellard_amd/csrc/stl_keycache.h
compiled by tests/native/hostemu_keycache.cpp): the check every x read from the
cache passes before it is used, the set / way hash, the victim choice, and the
verify workspace's layout with the cache's miss list in it.

  * for every golden key and 10,000 random ones, the decoder's own x passes
    iff the decoding is ok and x != 0, and what passes is that x exactly,
  * the wrong root, another key's x, single-bit flips, zero and random bytes
    are refused; x + p (where it fits) passes as the same value,
  * 2^20 random keys in the default geometry: at most 1 % lie in sets holding
    more keys than ways,
  * the workspace's sub-buffers lie inside verify_ws_bytes and do not overlap.
"""
import ctypes
import os

import numpy as np
import pytest

from tests.golden import ed25519_py as ed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "native", "libhostemu_keycache.so")
P = ed.P


def load_keycache_emu():
    from stellard_amd import build
    build.build_hostemu_keycache()
    lib = ctypes.CDLL(SO)
    V, Z = ctypes.c_void_p, ctypes.c_size_t
    lib.hostemu_kc_bound_violations.restype = ctypes.c_uint64
    lib.hostemu_kc_geometry.argtypes = [V]
    lib.hostemu_kc_decode.argtypes = [V, Z, V, V]
    lib.hostemu_kc_certify.argtypes = [V, V, Z, V, V]
    lib.hostemu_kc_index.argtypes = [V, Z, ctypes.c_uint32, V, V, V]
    lib.hostemu_kc_victim.restype = ctypes.c_uint32
    lib.hostemu_kc_victim.argtypes = [ctypes.c_uint32] * 3
    lib.hostemu_ws_layout.restype = ctypes.c_uint32
    lib.hostemu_ws_layout.argtypes = [ctypes.c_uint32, V, V, V]
    return lib


class KeyCacheEmu:
    def __init__(self):
        self.lib = load_keycache_emu()
        g = (ctypes.c_uint32 * 7)()
        self.lib.hostemu_kc_geometry(g)
        (self.log2_default, self.log2_min, self.log2_max, self.ways, self.set_bytes, self.tag_offset,
         self.x_offset) = list(g)

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def decode(self, keys):
        """-> (ok bool[n], canonical bytes of x(-A) uint8[n, 32])"""
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
        x = np.zeros_like(keys)
        ok = np.zeros(keys.shape[0], np.uint8)
        self.lib.hostemu_kc_decode(self._p(keys), keys.shape[0], self._p(x), self._p(ok))
        return ok.astype(bool), x

    def certify(self, keys, cand):
        """-> (pass bool[n], canonical bytes of the X returned uint8[n, 32])"""
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
        cand = np.ascontiguousarray(cand, np.uint8).reshape(-1, 32)
        assert keys.shape == cand.shape
        x = np.zeros_like(keys)
        ok = np.zeros(keys.shape[0], np.uint8)
        self.lib.hostemu_kc_certify(self._p(keys), self._p(cand), keys.shape[0], self._p(ok), self._p(x))
        return ok.astype(bool), x

    def index(self, keys, log2_sets=None, tags=False):
        """-> (set uint32[n], first way uint32[n]) with 2^log2_sets sets in
        use; with ``tags`` also the keys' tags as uint8[n, 8]"""
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
        k = self.log2_default if log2_sets is None else log2_sets
        s = np.zeros(keys.shape[0], np.uint32)
        w = np.zeros(keys.shape[0], np.uint32)
        t = np.zeros((keys.shape[0], 2), np.uint32)
        self.lib.hostemu_kc_index(self._p(keys), keys.shape[0], (1 << k) - 1, self._p(s), self._p(w), self._p(t))
        return (s, w, t.view(np.uint8).reshape(-1, 8)) if tags else (s, w)

    def victim(self, first_way, same, empty):
        return self.lib.hostemu_kc_victim(first_way, same, empty)


def crowding(sets, ways):
    """(keys that share their set with another key, keys in sets holding more than `ways`)"""
    _, inv, cnt = np.unique(sets, return_inverse=True, return_counts=True)
    per_key = cnt[inv]
    return int((per_key > 1).sum()), int((per_key > ways).sum())


def to_int(b):
    return int.from_bytes(bytes(b), "little")


def to_bytes(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


@pytest.fixture(scope="module")
def emu():
    return KeyCacheEmu()


@pytest.fixture(scope="module")
def keys(golden):
    """The golden keys (every adversarial class: small-order, mixed-order,
    non-canonical y, undecodable) and 10,000 seeded random 32-byte strings
    (about half of them decodable), each distinct key once."""
    rng = np.random.default_rng(0xCAC4E)
    k = np.concatenate([np.unique(golden["pk"], axis=0), rng.integers(0, 256, (10000, 32), np.uint8)])
    y1 = np.zeros((4, 32), np.uint8)  # y = 1 and y = p - 1 (x = 0), with either sign bit
    y1[0, 0] = y1[1, 0] = 1
    y1[1, 31] = 0x80
    y1[2] = to_bytes(P - 1)
    y1[3] = to_bytes(P - 1)
    y1[3, 31] |= 0x80
    return np.concatenate([k, y1])


@pytest.fixture(scope="module")
def decoded(emu, keys):
    return emu.decode(keys)


def test_geometry(emu):
    assert (emu.log2_default, emu.log2_min, emu.log2_max) == (20, 10, 24)
    assert emu.set_bytes == 256  # all a row gathers
    # six tags of 8 B, then six x of 32 B, inside the set
    assert emu.ways == 6 and emu.tag_offset + 8 * emu.ways <= emu.x_offset
    assert emu.x_offset + 32 * emu.ways == emu.set_bytes


def test_decoder_matches_python_reference(keys, decoded):
    """The harness's decoder is ge_frombytes_negate_vartime: ok and x(-A) as
    tests/golden/ed25519_py.py computes them (a sample: the big-integer powers are slow)."""
    ok, x = decoded
    idx = np.concatenate([np.arange(0, keys.shape[0], 37), np.arange(keys.shape[0] - 4, keys.shape[0])])
    for i in idx:
        v = to_int(keys[i])
        xa = ed.recover_x(v & ((1 << 255) - 1), v >> 255)
        assert ok[i] == (xa is not None), i
        if xa is not None:
            assert to_int(x[i]) == (P - xa) % P, i


def test_own_x_passes_iff_decodable_and_nonzero(emu, keys, decoded):
    ok, x = decoded
    nonzero = x.any(axis=1)
    assert ok.sum() > 4000 and (~ok).sum() > 4000  # both kinds are there
    assert (ok & ~nonzero).sum() >= 4  # y = +-1
    got, xc = emu.certify(keys, x)
    assert np.array_equal(got, ok & nonzero)
    assert np.array_equal(xc[got], x[got])
    assert emu.lib.hostemu_kc_bound_violations() == 0


def test_mutations_are_refused(emu, keys, decoded):
    ok, x = decoded
    good = ok & x.any(axis=1)
    k, xg = keys[good], x[good]
    n = k.shape[0]
    rng = np.random.default_rng(0xBAD)
    # the other root (wrong sign)
    wrong = np.stack([to_bytes(P - to_int(b)) for b in xg])
    assert not emu.certify(k, wrong)[0].any()
    # another key's x
    assert not emu.certify(k, np.roll(xg, 1, axis=0))[0].any()
    # all zero, random bytes
    assert not emu.certify(k, np.zeros_like(xg))[0].any()
    assert not emu.certify(k, rng.integers(0, 256, xg.shape, np.uint8))[0].any()
    # 64 single-bit flips of x (bits 0..254: bit 255 is not part of the value), each on every key
    for bit in rng.choice(255, 64, replace=False):
        f = xg.copy()
        f[:, bit >> 3] ^= np.uint8(1 << (bit & 7))
        assert not emu.certify(k, f)[0].any(), bit
    # x + p where it fits in 255 bits (x < 19): the same value.  Keys with such an
    # x(-A): y^2 = (1 + x^2) / (1 - d x^2) where that is a square, the sign bit of x(A) = p - x
    sk, sx = [], []
    for xs in range(1, 19):
        yy = (1 + xs * xs) * ed.inv((1 - ed.D * xs * xs) % P) % P
        y = pow(yy, (P + 3) // 8, P)
        if y * y % P != yy:
            y = y * ed.SQRTM1 % P
        if y * y % P != yy:
            continue
        sk.append(to_bytes(y | (((P - xs) & 1) << 255)))
        sx.append(to_bytes(xs))
    assert len(sk) >= 4
    sk, sx = np.stack(sk), np.stack(sx)
    dok, dx = emu.decode(sk)
    assert dok.all() and np.array_equal(dx, sx)
    plus = np.stack([to_bytes(to_int(b) + P) for b in sx])
    got, xc = emu.certify(sk, plus)
    assert got.all() and np.array_equal(xc, sx)
    # a key that does not decode passes with nothing: its own decoder output, zero, random
    bad = keys[~ok]
    assert not emu.certify(bad, x[~ok])[0].any()
    assert not emu.certify(bad, rng.integers(0, 256, bad.shape, np.uint8))[0].any()
    assert emu.lib.hostemu_kc_bound_violations() == 0


def test_victim_choice(emu):
    W = emu.ways
    every = (1 << W) - 1
    for first in range(W):
        assert emu.victim(first, 0, 0) == first  # full set: the hash's way
        assert emu.victim(first, 0, every) == first  # empty set: the hash's way
        for w in range(W):
            assert emu.victim(first, 1 << w, every) == w  # the key's own slot before any empty one
            assert emu.victim(first, 0, 1 << w) == w  # the only empty way
        assert emu.victim(first, 0b101010, 0b010101) == 1  # of several slots with the tag, the one a lookup tries
        # the nearest empty way counting up from the hash's way
        assert emu.victim(first, 0, every & ~(1 << first)) == (first + 1) % W


def test_occupancy_of_the_default_geometry(emu):
    """2^20 random keys into the default 2^20 sets: at most 1 % of them may lie
    in sets that hold more keys than ways.  For an ideal hash the sets are
    Poisson(1): sum over k > W of k e^-1 / k! of the keys are in such sets,
    1.90 % for W = 4 (measured with this hash: 1.86 %, which is why a set has
    six tagged slots, not four with the key's bytes) and 0.06 % for W = 6.
    The first ways spread evenly, and the tags do not follow the set index."""
    rng = np.random.default_rng(0x0CC)
    k = rng.integers(0, 256, (1 << 20, 32), np.uint8)
    sets, ways, tags = emu.index(k, tags=True)
    assert sets.max() < (1 << 20)
    _, over = crowding(sets, emu.ways)
    print("keys in sets over", emu.ways, "ways:", over, over / (1 << 20), "over 4:", crowding(sets, 4)[1] / (1 << 20))
    assert over <= (1 << 20) // 100
    share = np.bincount(ways, minlength=emu.ways) / (1 << 20)
    assert ways.max() < emu.ways and np.all(np.abs(share - 1 / emu.ways) < 0.01)
    # keys that meet in a set differ in their tags (64 bits: no pair among 2^20 keys agrees)
    both = np.concatenate([sets[:, None].astype(np.uint64), tags.view(np.uint64)], axis=1)
    assert np.unique(both, axis=0).shape[0] == (1 << 20)
    # a masked index is the low bits of the full one
    s4, _ = emu.index(k[:1000], 4)
    assert np.array_equal(s4, sets[:1000] & 15)


def gpu_test_seeds(n=4096):
    """The signers' seeds of tests/test_gpu_keycache.py's cold / warm batch."""
    return np.random.default_rng(0x6EC).integers(0, 256, (n, 32), np.uint8)


def test_gpu_batch_keys_fit_their_sets(emu):
    """The 4,096 keys of the GPU test's cold / warm batch are distinct and no
    set of the default geometry holds more of them than it has ways, so that
    test may ask for no miss at all once the cache is warm."""
    from tests import oracle_bind
    seeds = gpu_test_seeds()
    n = seeds.shape[0]
    pk, _, _ = oracle_bind.hostemu_sign_adversarial(oracle_bind.load_hostemu(), seeds, np.zeros((n, 32), np.uint8),
                                                    np.zeros(n, np.uint8), np.zeros(n, np.uint32))
    assert np.unique(pk, axis=0).shape[0] == n
    sets, _ = emu.index(pk)
    shared, over = crowding(sets, emu.ways)
    print("keys sharing a set:", shared, "in sets over the ways:", over)
    assert over == 0


@pytest.mark.parametrize("grid", [1, 64, 1280, 2560])
def test_workspace_layout(emu, grid):
    off = (ctypes.c_uint64 * 14)()
    size = (ctypes.c_uint64 * 14)()
    total = (ctypes.c_uint64 * 2)()
    assert emu.lib.hostemu_ws_layout(grid, off, size, total) == 14
    off, size = list(off), list(size)
    for dedup, count in ((False, 6), (True, 14)):
        spans = sorted((off[i], off[i] + size[i]) for i in range(count))
        assert spans[0][0] == 0
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a1 <= b0, (grid, dedup)  # no overlap
        assert spans[-1][1] <= total[1 if dedup else 0], (grid, dedup)
        assert all(o % 16 == 0 for o in off[:count])
    # the key domain starts where the workspace without it ends
    assert off[6] == total[0] and total[1] > total[0]
