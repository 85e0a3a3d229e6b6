"""GPU tests of the decoded-key cache (stl_keycache.h, STL_TUNE_KEY_CACHE): a
cold call misses every row and later calls hit; whatever the cache holds --
evicted, overwritten by another stream, poisoned -- the accept bits are exact.

Every call uses STL_ONE_LANE (small batches then take the one-lane phase 1 the
cache serves) and STL_NO_AUTO_DEDUP (repeated keys stay on that path).

Run on an MI355X:  python -u -m pytest tests/test_gpu_keycache.py -m gpu -x -v
"""
import threading

import numpy as np
import pytest

from tests.golden import ed25519_py as ed
from tests.test_keycache_host import KeyCacheEmu, crowding, gpu_test_seeds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def stl(torch_cuda):
    from stellard_amd import verify
    verify.init()
    return verify


@pytest.fixture(scope="module")
def emu():
    return KeyCacheEmu()


def _cuda(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _flags(stl):
    return stl.ONE_LANE | stl.NO_AUTO_DEDUP


class knob:
    """STL_TUNE_KEY_CACHE set for a block; on leaving, the knob is back and the cache empty."""

    def __init__(self, stl, value=None):
        self.stl, self.value = stl, value

    def __enter__(self):
        self.prev = self.stl.debug_tuning(self.stl.TUNE_KEY_CACHE, -1)
        if self.value is not None:
            self.stl.debug_tuning(self.stl.TUNE_KEY_CACHE, self.value)
        self.stl.key_cache_clear()
        return self

    def __exit__(self, *exc):
        self.stl.debug_tuning(self.stl.TUNE_KEY_CACHE, self.prev)
        self.stl.key_cache_clear()


def _verify(stl, torch, d, n, stream=None):
    """One call -> (bits, hits, misses of this call)."""
    before = stl.get_stats()
    words = stl.verify_batch_device(*d, policy=_flags(stl), stream=stream)
    torch.cuda.synchronize()
    after = stl.get_stats()
    return (stl.words_to_bool(words, n), after["key_cache_hits"] - before["key_cache_hits"],
            after["key_cache_misses"] - before["key_cache_misses"])


def _golden_rows(golden, n, seed):
    idx = np.random.default_rng(seed).integers(0, golden["sig"].shape[0], n)
    return (golden["sig"][idx], golden["msg"][idx], golden["pk"][idx],
            golden["expected_sodium_1_0_18"][idx].astype(bool))


def test_settings_report_the_cache(stl):
    info = stl.key_cache_info()
    assert info["ways"] == 6 and info["bytes"] == 256 << info["sets_log2"] and info["ptr"]
    assert stl.execution_settings()["key_cache"] == info["sets_log2"]


def test_cold_then_warm(stl, torch_cuda, emu):
    """4,096 GPU-signed rows over distinct keys, 1 % with a flipped message."""
    torch = torch_cuda
    n = 4096
    rng = np.random.default_rng(0x6ED)
    seeds = gpu_test_seeds(n)
    msgs = rng.integers(0, 256, (n, 32), np.uint8)
    dseed, dmsg = _cuda(torch, seeds, msgs)
    pk, sig = stl.sign_batch_device(dseed, dmsg)
    bad = rng.choice(n, n // 100, replace=False)
    exp = np.ones(n, bool)
    exp[bad] = False
    dmsg[torch.from_numpy(bad).cuda(), 0] ^= 1
    torch.cuda.synchronize()
    d = (sig, dmsg, pk)
    info = stl.key_cache_info()
    sets, _ = emu.index(pk.cpu().numpy(), info["sets_log2"])
    shared, over = crowding(sets, info["ways"])
    with knob(stl):
        bits, hits, misses = _verify(stl, torch, d, n)
        assert np.array_equal(bits, exp)
        assert (hits, misses) == (0, n)
        seen = []
        for call in (2, 3, 4):
            bits, hits, misses = _verify(stl, torch, d, n)
            assert np.array_equal(bits, exp), call
            assert hits + misses == n, call
            seen.append(misses)
        print("misses of calls 2-4:", seen, "keys sharing a set:", shared, "in sets over the ways:", over)
        assert seen[0] <= shared
        assert seen[2] <= over


@pytest.mark.parametrize("value", [None, 4])
def test_goldens_through_the_cache(stl, torch_cuda, golden, value):
    """Every adversarial class, with the whole cache and with 16 sets (constant eviction)."""
    sig, msg, pk, exp = _golden_rows(golden, 5000, seed=21)
    d = _cuda(torch_cuda, sig, msg, pk)
    with knob(stl, value):
        total = 0
        for call in range(3):
            bits, hits, misses = _verify(stl, torch_cuda, d, 5000)
            assert np.array_equal(bits, exp), (value, call)
            assert hits + misses == 5000
            total += hits
        assert value is not None or total > 0  # with every set in use, repeated keys hit


def test_concurrent_overwrite(stl, torch_cuda, golden):
    """Two threads on two streams, 16 sets: each overwrites what the other looks up."""
    torch = torch_cuda
    n = 20000
    sig, msg, pk, exp = _golden_rows(golden, n, seed=22)
    d = _cuda(torch, sig, msg, pk)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = [[], []]
    err = []

    def worker(k):
        try:
            torch.cuda.set_device(0)
            for _ in range(5):
                w = stl.verify_batch_device(*d, policy=_flags(stl), stream=streams[k])
                streams[k].synchronize()
                out[k].append(stl.words_to_bool(w, n))
        except Exception as e:  # noqa: BLE001 - reported by the asserting thread
            err.append(e)

    try:
        with knob(stl, 4):
            ts = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            torch.cuda.synchronize()
            assert not err, err
            for k in range(2):
                assert len(out[k]) == 5
                for bits in out[k]:
                    assert np.array_equal(bits, exp)
    finally:
        for s in streams:
            stl.release_stream(s)


def test_poisoned_cache(stl, torch_cuda, emu):
    """Every way of each key's set holds {the key's tag, the wrong root}, then
    {the key's tag, random bytes}: no row may hit, and the bits are exact.  The cache keeps
    x(-A) = p - x(A); the wrong root is p minus that, x(A) itself, computed by
    tests/golden/ed25519_py.py."""
    torch = torch_cuda
    n = 512
    rng = np.random.default_rng(0x9015)
    dseed, dmsg = _cuda(torch, rng.integers(0, 256, (n, 32), np.uint8), rng.integers(0, 256, (n, 32), np.uint8))
    pk, sig = stl.sign_batch_device(dseed, dmsg)
    dmsg[::7, 0] ^= 1
    torch.cuda.synchronize()
    exp = np.ones(n, bool)
    exp[::7] = False
    hpk = pk.cpu().numpy()
    wrong = np.zeros((n, 32), np.uint8)
    for i in range(n):
        v = int.from_bytes(bytes(hpk[i]), "little")
        xa = ed.recover_x(v & ((1 << 255) - 1), v >> 255)
        assert xa
        wrong[i] = np.frombuffer(xa.to_bytes(32, "little"), np.uint8)
    info = stl.key_cache_info()
    sets, _, tags = emu.index(hpk, info["sets_log2"], tags=True)
    shared, _ = crowding(sets, info["ways"])  # keys that meet another in their set (a few of 512 at most)
    # the cache as a (sets, 256) byte tensor over the library's allocation
    nbytes = info["bytes"]
    assert nbytes == (emu.set_bytes << info["sets_log2"]) and info["ways"] == emu.ways
    cache = _device_view(torch, info["ptr"], nbytes).view(1 << info["sets_log2"], emu.set_bytes)
    dsets = torch.from_numpy(sets.astype(np.int64)).cuda()
    with knob(stl):
        for poison in (wrong, rng.integers(0, 256, (n, 32), np.uint8)):
            stl.key_cache_clear()
            rows = np.zeros((n, emu.set_bytes), np.uint8)
            for w in range(emu.ways):
                rows[:, emu.tag_offset + 8 * w:emu.tag_offset + 8 * w + 8] = tags
                rows[:, emu.x_offset + 32 * w:emu.x_offset + 32 * w + 32] = poison
            cache[dsets] = torch.from_numpy(rows).cuda()
            torch.cuda.synchronize()
            bits, hits, misses = _verify(stl, torch, (sig, dmsg, pk), n)
            assert np.array_equal(bits, exp)
            assert (hits, misses) == (0, n)
            # the misses replaced the poison where lookups find it: now the rows hit
            # (but for keys that share their set with another one)
            bits, hits, misses = _verify(stl, torch, (sig, dmsg, pk), n)
            assert np.array_equal(bits, exp)
            assert hits + misses == n and misses <= shared


def _device_view(torch, ptr, nbytes):
    """A uint8 CUDA tensor over device memory the library owns (no copy, no ownership)."""
    class _Mem:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    return torch.as_tensor(_Mem(), device="cuda")


def test_knob_off(stl, torch_cuda, golden):
    sig, msg, pk, exp = _golden_rows(golden, 5000, seed=23)
    d = _cuda(torch_cuda, sig, msg, pk)
    with knob(stl, 0):
        assert stl.execution_settings()["key_cache"] == 0
        for _ in range(2):
            bits, hits, misses = _verify(stl, torch_cuda, d, 5000)
            assert np.array_equal(bits, exp)
            assert (hits, misses) == (0, 0)
