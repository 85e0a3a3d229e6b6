"""GPU tests of the decoded-key cache's lookup inside verify_prep_kernel, of
key_cache_fill_kernel finishing the missed rows, and of the second-choice set:
waves whose lanes hit and miss side by side, missed rows' fallback flags,
chunk tails, a primary set that eight keys share, and constant eviction
through both sets.  The accept bits are exact in every call.

Every call uses STL_ONE_LANE (small batches then take the one-lane phase 1 the
cache serves) and STL_NO_AUTO_DEDUP (repeated keys stay on that path).

Run on an MI355X:  python -u -m pytest tests/test_gpu_keycache_fused.py -m gpu -x -v
"""
import numpy as np
import pytest

from tests.test_gpu_keycache import _cuda, _golden_rows, knob
from tests.test_keycache_alt_host import CROWDED_LOG2, KeyCacheAltEmu, crowded_batch

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


def _verify(stl, torch, d, n, extra=0):
    """One call -> (bits, hits, misses of this call)."""
    before = stl.get_stats()
    words = stl.verify_batch_device(*d, policy=stl.ONE_LANE | stl.NO_AUTO_DEDUP | extra)
    torch.cuda.synchronize()
    after = stl.get_stats()
    return (stl.words_to_bool(words, n), after["key_cache_hits"] - before["key_cache_hits"],
            after["key_cache_misses"] - before["key_cache_misses"])


@pytest.mark.parametrize("full_length", [False, True])
def test_mixed_waves(stl, torch_cuda, golden, full_length):
    """The even rows' keys are cached, the odd rows' mostly not: every wave
    holds lanes that finish in prep beside lanes the fill kernel finishes.
    With STL_FULL_LENGTH every ok row is a fallback row, so the missed rows'
    flags reach the fallback words through the fill kernel's atomics."""
    n = 5000
    sig, msg, pk, exp = _golden_rows(golden, n, seed=31)
    extra = stl.FULL_LENGTH if full_length else 0
    with knob(stl, 0):
        off, hits, misses = _verify(stl, torch_cuda, _cuda(torch_cuda, sig, msg, pk), n, extra)
        assert (hits, misses) == (0, 0)
    assert np.array_equal(off, exp)
    even = _cuda(torch_cuda, sig[::2], msg[::2], pk[::2])
    every = _cuda(torch_cuda, sig, msg, pk)
    with knob(stl):
        bits, hits, misses = _verify(stl, torch_cuda, even, n // 2, extra)
        assert np.array_equal(bits, exp[::2])
        assert (hits, misses) == (0, n // 2)
        bits, hits, misses = _verify(stl, torch_cuda, every, n, extra)
        print("mixed call: hits", hits, "misses", misses)
        assert np.array_equal(bits, exp) and np.array_equal(bits, off)
        assert hits + misses == n
        assert hits > 0 and misses > 0


@pytest.mark.parametrize("n", [1, 63, 65, 4097])
def test_tails(stl, torch_cuda, golden, n):
    sig, msg, pk, exp = _golden_rows(golden, n, seed=32 + n)
    d = _cuda(torch_cuda, sig, msg, pk)
    with knob(stl):
        bits, hits, misses = _verify(stl, torch_cuda, d, n)
        assert np.array_equal(bits, exp)
        assert (hits, misses) == (0, n)
        bits, hits, misses = _verify(stl, torch_cuda, d, n)
        assert np.array_equal(bits, exp)
        assert hits + misses == n


def test_crowded_set(stl, torch_cuda):
    """Eight keys in one primary set of six ways (tests/test_keycache_alt_host.py
    selects them): only the alternate sets let every row hit.  Inserts racing
    within a call may need a few calls to settle."""
    torch = torch_cuda
    got = crowded_batch(KeyCacheAltEmu())
    assert got is not None
    seeds, _ = got
    n = seeds.shape[0]
    rng = np.random.default_rng(0xC40E)
    dseed, dmsg = _cuda(torch, seeds, rng.integers(0, 256, (n, 32), np.uint8))
    pk, sig = stl.sign_batch_device(dseed, dmsg)
    dmsg[::9, 0] ^= 1
    torch.cuda.synchronize()
    exp = np.ones(n, bool)
    exp[::9] = False
    seen = []
    with knob(stl, CROWDED_LOG2):
        for call in range(10):
            bits, hits, misses = _verify(stl, torch, (sig, dmsg, pk), n)
            assert np.array_equal(bits, exp), call
            assert hits + misses == n, call
            seen.append(misses)
            if misses == 0:
                break
    print("misses per call:", seen)
    assert seen[0] == n and seen[-1] == 0


def test_16_sets(stl, torch_cuda, golden):
    """Constant eviction through both sets."""
    n = 20000
    sig, msg, pk, exp = _golden_rows(golden, n, seed=33)
    d = _cuda(torch_cuda, sig, msg, pk)
    with knob(stl, 4):
        for call in range(3):
            bits, hits, misses = _verify(stl, torch_cuda, d, n)
            assert np.array_equal(bits, exp), call
            assert hits + misses == n, call
