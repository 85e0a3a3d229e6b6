"""GPU tests of the verified-ID cache (stl_sigcache_*): whatever the cache
holds, the cached blob call writes the bits, status and IDs of
stl_signed_blob_verify_batch_device, which are the oracle's; a hit needs the
whole ID, so no mutated blob ever hits; hits and verified count what they say.

Every check compares three things: the uncached call on the same buffers, the
cached call, and oracle.signed_blob_verify_batch.

Run on an MI355X:  python -u -m pytest tests/test_gpu_sigcache.py -m gpu -x -v
"""
import ctypes
import threading

import numpy as np
import pytest

from tests import signer_cases as SC
from tests import sigcache_py as SP
from tests import txblob

pytestmark = pytest.mark.gpu

L = 2**252 + 27742317777372353535851937790883648493
GUARD = 0xA5


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


class Batch:
    """Blobs in device memory, and what the oracle says about them."""

    def __init__(self, stl, torch, oracle, blobs, kind=0, policy=0, exp=None):
        from stellard_amd.verify import _pack
        self.blobs, self.n, self.kind = list(blobs), len(blobs), kind
        buf, offs, lens = _pack(self.blobs)
        self.dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda()
                    for a in (buf, offs.view(np.int64), lens.view(np.int32))]
        self.exp, self.exp_ids = exp if exp is not None else oracle.signed_blob_verify_batch(
            kind, self.blobs, policy=policy, ids=True)


def run(torch, stl, call, b, flags=0, ids=True, stream=None, **kw):
    """One blob call on guarded buffers -> (bits, status, ids or None, out)."""
    n, nw = b.n, (b.n + 63) // 64
    words = torch.full((nw + 2,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    status = torch.full((n + 64,), GUARD, dtype=torch.uint8, device="cuda")
    idt = torch.full((n + 2, 32), GUARD, dtype=torch.uint8, device="cuda") if ids else None
    torch.cuda.synchronize()
    out = call(*b.dev, out_words=words[:nw], out_status=status[:n], out_ids=idt[:n] if ids else None,
               stream=stream, **kw, **({"policy": flags} if call is stl.signed_blob_verify_batch_device
                                       else {"flags": flags}))
    torch.cuda.synchronize()
    assert (words[nw:] == -0x5A5A5A5A5A5A5A5B).all() and (status[n:] == GUARD).all(), "guard bytes overwritten"
    if ids:
        assert (idt[n:] == GUARD).all(), "guard bytes past the IDs overwritten"
    return (stl.words_to_bool(words[:nw], n), status[:n].cpu().numpy(), idt[:n].cpu().numpy() if ids else None, out)


def uncached(torch, stl, b, flags=0, **kw):
    return run(torch, stl, stl.signed_blob_verify_batch_device, b, flags, kind=b.kind, **kw)


def check(torch, stl, cache, b, flags=0, ids=True, stream=None):
    """The cached call against the uncached call on the same buffers and the
    oracle -> (bits, status, ids, hits, verified)."""
    rb, rs, ri, _ = uncached(torch, stl, b, flags, stream=stream)
    cb, cs, ci, out = run(torch, stl, cache.signed_blob_verify_batch_device, b, flags, ids=ids, stream=stream)
    assert np.array_equal(cb, rb), np.nonzero(cb != rb)[0][:10]
    assert np.array_equal(cs, rs)
    if ids:
        assert np.array_equal(ci, ri)
    if b.exp is not None:
        # a DEFERRED row is the host's to decide (stl.h: the device writes bit 0 and a zero ID), and the
        # oracle does decide it -- it accepts a payment cut short inside its last, unsigned field
        dec = rs != stl.TX_DEFERRED
        assert np.array_equal(cb[dec], b.exp[dec]), np.nonzero(dec & (cb != b.exp))[0][:10]
        ok = rs == stl.TX_OK
        assert np.array_equal(ri[ok], b.exp_ids[ok])
    assert not cb[rs != stl.TX_OK].any()
    return cb, rs, ri, out["hits"], out["verified"]


def present(torch, stl, cache, ids, stream=None):
    t = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
    n = ids.shape[0]
    nw = (n + 63) // 64
    words = torch.full((nw + 1,), 0x77, dtype=torch.int64, device="cuda")
    cache.lookup_device(t, out_words=words[:nw], stream=stream)
    torch.cuda.synchronize()
    assert int(words[nw]) == 0x77
    if n % 64:
        assert int(words[nw - 1]) >> (n % 64) == 0  # the tail bits are zero
    return stl.words_to_bool(words[:nw], n)


def flip(rng, blob, pos=None):
    b = bytearray(blob)
    pos = int(rng.integers(0, len(b))) if pos is None else pos
    b[pos] ^= 1 << int(rng.integers(0, 8))
    return bytes(b)


@pytest.fixture(scope="module")
def corpus(stl, torch_cuda, oracle):
    """About 2,000 blobs: every class of signer_cases (random signatures: the
    decidable ones are rejects; deferred and malformed rows), correctly signed
    payments, copies of those with one flipped bit or a truncation, and blobs
    repeated inside the batch -- shuffled; and a seed under which no set of a
    2^16-set cache receives more than four accepted IDs."""
    rng = np.random.default_rng(0x51C)
    cases = [c.blob for c in SC.make_cases(40 * len(SC.CLASSES), 0x51C0)]
    good = txblob.valid_corpus(oracle, 900, 0x51C1)
    bad = [flip(rng, g) if i % 3 else g[: int(rng.integers(1, len(g)))] for i, g in enumerate(good[:300])]
    repeats = good[:60] + cases[:30] + bad[:10]
    blobs = cases + good + bad + repeats
    order = rng.permutation(len(blobs))
    blobs = [blobs[i] for i in order]
    b = Batch(stl, torch_cuda, oracle, blobs)
    b.good = good
    # the oracle also decides the rows the device defers to the host (check() has the reason): from here
    # on exp is the oracle's bit where the device decides, 0 on the handful of rows it defers
    _, status, _, _ = uncached(torch_cuda, stl, b)
    deferred_accepts = b.exp & (status == stl.TX_DEFERRED)
    assert deferred_accepts.sum() <= 5
    b.exp = b.exp & ~deferred_accepts
    accepted =[b.exp_ids[i].tobytes() for i in np.nonzero(b.exp)[0]]
    b.seed = SP.seed_without_overfull_set(accepted, 16, first=0x5EED)
    return b


def cycled(stl, torch, oracle, corpus, n, start=0):
    """n rows of the corpus from ``start`` on, wrapping."""
    idx = (start + np.arange(n)) % corpus.n
    return Batch(stl, torch, oracle, [corpus.blobs[i] for i in idx], exp=(corpus.exp[idx], corpus.exp_ids[idx]))


# ---- 1. cold then warm ----
def test_cold_then_warm(stl, torch_cuda, oracle, corpus):
    torch = torch_cuda
    b = corpus
    assert 1900 <= b.n <= 2300
    accepted_ids = {b.exp_ids[i].tobytes() for i in np.nonzero(b.exp)[0]}
    assert SP.max_set_load(accepted_ids, b.seed, 16) <= SP.WAYS and b.seed != 0
    with stl.SigCache(16, seed=b.seed) as c:
        bits, status, ids, hits, verified = check(torch, stl, c, b)
        ok = status == stl.TX_OK
        assert set(np.unique(status)) == {stl.TX_OK, stl.TX_DEFERRED, stl.TX_MALFORMED}
        assert bits.sum() >= 900 and (ok & ~bits).sum() >= 500
        assert hits == 0 and verified == int(ok.sum())
        bits2, status2, ids2, hits, verified = check(torch, stl, c, b)
        assert np.array_equal(bits2, bits)
        assert hits == int((ok & bits).sum()) and verified == int((ok & ~bits).sum())
        # the bare lookup: the accept bitmap on the decidable rows, 0 elsewhere
        there = present(torch, stl, c, ids)
        assert np.array_equal(there, bits & ok)
        # a third call, without the IDs: the same counts
        _, _, _, h3, v3 = check(torch, stl, c, b, ids=False)
        assert (h3, v3) == (hits, verified)


# ---- 2. edges ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_edges(stl, torch_cuda, oracle, corpus, n):
    """The 64-lane wave and the 256-lane workgroup of the probe, gather,
    scatter and insert kernels; 4,099 rows wrap the corpus (every blob twice)."""
    torch = torch_cuda
    b = cycled(stl, torch, oracle, corpus, n, start=7 * n)
    acc = np.nonzero(b.exp)[0]
    half = Batch(stl, torch, oracle, [b.blobs[i] for i in acc[::2]]) if len(acc) else None
    seen = {b.blobs[i] for i in acc[::2]}
    want_hits = sum(1 for i in acc if b.blobs[i] in seen)
    stream = torch.cuda.Stream()
    for variant in ("half_warm", "stream", "no_ids"):
        with stl.SigCache(16, seed=corpus.seed) as c:
            s = stream if variant == "stream" else None
            if half is not None:
                check(torch, stl, c, half, stream=s)
            bits, status, _, hits, verified = check(torch, stl, c, b, ids=variant != "no_ids", stream=s)
            ok = status == stl.TX_OK
            assert hits == want_hits and verified == int(ok.sum()) - want_hits, (n, variant)
            _, _, _, hits, verified = check(torch, stl, c, b, ids=variant != "no_ids", stream=s)
            assert hits == int((ok & bits).sum()) and verified == int((ok & ~bits).sum()), (n, variant)


# ---- 3. a hit is never a forgery ----
def test_a_mutated_blob_never_hits(stl, torch_cuda, oracle, corpus):
    torch = torch_cuda
    rng = np.random.default_rng(3)
    good = corpus.good[:300]
    warm = Batch(stl, torch, oracle, good)
    assert warm.exp.all()
    mutated = []
    for i, g in enumerate(good):
        # the last byte, a byte of the signature (field 0x74, 64 bytes), of the key (0x73, 32 bytes), of the body
        sig_at, pk_at = g.find(b"\x74\x40") + 2, g.find(b"\x73\x20") + 2
        assert sig_at >= 2 and pk_at >= 2
        pos = [len(g) - 1, sig_at + int(rng.integers(0, 64)), pk_at + int(rng.integers(0, 32)),
               int(rng.integers(0, len(g)))][i % 4]
        mutated.append(flip(rng, g, pos))
    m = Batch(stl, torch, oracle, mutated)
    with stl.SigCache(16, seed=corpus.seed) as c:
        _, _, _, hits, verified = check(torch, stl, c, warm)
        assert (hits, verified) == (0, 300)
        _, _, _, hits, _ = check(torch, stl, c, warm)
        assert hits == 300
        bits, status, ids, hits, verified = check(torch, stl, c, m)
        assert hits == 0 and verified == int((status == stl.TX_OK).sum())
        assert not bits.all()
        # the few mutants that still verify (a flipped bit outside what is signed or checked) are new IDs
        assert not (set(map(bytes, ids[bits])) & set(map(bytes, warm.exp_ids)))


def test_rejects_are_never_cached(stl, torch_cuda, oracle, corpus):
    torch = torch_cuda
    rows = [blob for blob, e in zip(corpus.blobs, corpus.exp) if not e][:700]
    b = Batch(stl, torch, oracle, rows)
    assert not b.exp.any()
    with stl.SigCache(16, seed=corpus.seed) as c:
        for _ in range(2):
            bits, status, ids, hits, verified = check(torch, stl, c, b)
            assert hits == 0 and verified == int((status == stl.TX_OK).sum()) > 300
            assert set(np.unique(status)) == {stl.TX_OK, stl.TX_DEFERRED, stl.TX_MALFORMED}
            assert not present(torch, stl, c, ids).any()


# ---- 4. eviction ----
def test_eviction_in_a_one_set_cache(stl, torch_cuda, oracle, corpus):
    torch = torch_cuda
    nine = corpus.good[300:309]
    ones = [Batch(stl, torch, oracle, [g]) for g in nine]
    allb = Batch(stl, torch, oracle, nine)
    assert allb.exp.all() and len({i.tobytes() for i in allb.exp_ids}) == 9
    with stl.SigCache(0, seed=corpus.seed) as c:
        assert c.info()["bytes"] == 128
        for one in ones:
            bits, _, _, hits, verified = check(torch, stl, c, one)
            assert bits.all() and (hits, verified) == (0, 1)
        there = present(torch, stl, c, allb.exp_ids)
        assert there.sum() <= 4 and there[8]
        _, _, _, hits, verified = check(torch, stl, c, allb)
        assert hits == int(there.sum()) and hits + verified == 9
        _, _, _, hits, verified = check(torch, stl, c, allb)
        assert 0 < hits <= 4 and hits + verified == 9


# ---- 5. predicate binding ----
def test_predicate_binding(stl, torch_cuda, oracle):
    from stellard_amd import _native as N
    torch = torch_cuda
    rng = np.random.default_rng(5)
    pk, sk = oracle.keypair(rng.bytes(32))

    def sign_plus_l(h, sk_):
        sig = oracle.sign(h, sk_)
        return sig[:32] + (int.from_bytes(sig[32:], "little") + L).to_bytes(32, "little")

    fields = txblob.payment_fields(rng, pk, 1)
    blob, h, sig = txblob.signed_blob(fields, sk, sign_plus_l)
    honest, _, _ = txblob.signed_blob(txblob.payment_fields(rng, pk, 2), sk, oracle.sign)
    raw = N.STL_POLICY_STELLARD_1_0_0 | N.STL_DEBUG_RAW_PREDICATE
    assert oracle.verify_raw(sig, h, pk, policy=1) and not oracle.verify(sig, h, pk, policy=1)
    # the oracle's composite predicate rejects S + L under both policies: exp is for the default caches
    b = Batch(stl, torch, oracle, [blob, honest])
    assert list(b.exp) == [False, True]
    with stl.SigCache(4, policy=raw, seed=9) as c:
        assert c.info()["predicate"] == raw
        b.exp = None  # the raw predicate: the oracle's statement is verify_raw above
        bits, _, ids, hits, verified = check(torch, stl, c, b, flags=raw)
        assert bits.all() and (hits, verified) == (0, 2)
        bits, _, _, hits, verified = check(torch, stl, c, b, flags=raw | N.STL_FULL_LENGTH)
        assert bits.all() and (hits, verified) == (2, 0)
        assert present(torch, stl, c, ids).all()
        for flags in (0, N.STL_POLICY_STELLARD_1_0_0, N.STL_DEBUG_RAW_PREDICATE):
            with pytest.raises(N.StlError) as e:
                c.signed_blob_verify_batch_device(*b.dev, flags=flags)
            assert e.value.rc == N.STL_EINVAL
    b = Batch(stl, torch, oracle, [blob, honest])
    for policy in (0, N.STL_POLICY_STELLARD_1_0_0):
        b.exp = oracle.signed_blob_verify_batch(0, b.blobs, policy=policy)
        with stl.SigCache(4, policy=policy, seed=9) as c:
            for hits_want in ((0, 2), (1, 1)):
                bits, _, ids, hits, verified = check(torch, stl, c, b, flags=policy)
                assert list(bits) == [False, True] and (hits, verified) == hits_want
            assert list(present(torch, stl, c, ids)) == [False, True]
            with pytest.raises(N.StlError) as e:
                c.signed_blob_verify_batch_device(*b.dev, flags=raw)
            assert e.value.rc == N.STL_EINVAL


# ---- 6. validations ----
def test_validations(stl, torch_cuda, oracle):
    """The 600-validation recipe of test_gpu_keyset_by_key (6 validators, some
    blobs with a flipped bit or truncated) plus 4 transactions, which a
    validation cache must call malformed or reject."""
    torch = torch_cuda
    rng = np.random.default_rng(51)
    keys = [oracle.keypair(rng.bytes(32)) for _ in range(6)]
    blobs = []
    for i in range(600):
        pk, sk = keys[i % 6]
        fs = txblob.validation_fields(rng, pk, full=bool(i % 2))
        b, _, _ = txblob.signed_validation(fs, sk, oracle.sign)
        x = rng.random()
        if x < 0.15:
            b = flip(rng, b)
        elif x < 0.2:
            b = b[: int(rng.integers(1, len(b)))]
        blobs.append(b)
    blobs += txblob.valid_corpus(oracle, 4, 52)
    b = Batch(stl, torch, oracle, blobs, kind=1)
    assert b.exp[:600].sum() > 400 and not b.exp[600:].any()
    seed = SP.seed_without_overfull_set([b.exp_ids[i].tobytes() for i in np.nonzero(b.exp)[0]], 12, first=77)
    with stl.SigCache(12, kind=stl.BLOB_VALIDATION, seed=seed) as c:
        assert c.info()["kind"] == stl.BLOB_VALIDATION
        bits, status, ids, hits, verified = check(torch, stl, c, b)
        ok = status == stl.TX_OK
        assert hits == 0 and verified == int(ok.sum())
        _, _, _, hits, verified = check(torch, stl, c, b)
        assert hits == int(bits.sum()) > 400 and verified == int((ok & ~bits).sum())


# ---- 7. injected errors ----
def test_fault_injection(stl, torch_cuda, oracle, corpus):
    """Every HIP call of one cached call on a half-warm 257-row batch, failed
    in turn: the call returns < 0, nothing that was not accepted is in the
    cache afterwards, and the next clean call gives the right bits."""
    from stellard_amd import _native as N
    torch = torch_cuda
    b = cycled(stl, torch, oracle, corpus, 257, start=100)
    acc = np.nonzero(b.exp)[0]
    half = Batch(stl, torch, oracle, [b.blobs[i] for i in acc[::2]])
    assert len(acc) > 60
    rb, rs, ri, _ = uncached(torch, stl, b)
    assert np.array_equal(rb, b.exp)
    seen = {b.blobs[i] for i in acc[::2]}
    want_hits = sum(1 for i in acc if b.blobs[i] in seen)
    stream = torch.cuda.Stream()  # a fresh context: the first calls also allocate
    failed, k = 0, 0
    with stl.SigCache(16, seed=corpus.seed) as c, torch.cuda.stream(stream):
        try:
            while True:
                assert k < 96, "the countdown never ran out"
                c.clear()
                if k:  # the very first call meets an empty context and an empty cache
                    c.signed_blob_verify_batch_device(*half.dev)
                torch.cuda.synchronize()
                stl.debug_fault_after(k)
                k += 1
                try:
                    out = c.signed_blob_verify_batch_device(*b.dev, tx_ids=True)
                except N.StlError as e:
                    assert e.rc < 0
                    failed += 1
                    stl.debug_fault_after(-1)
                    torch.cuda.synchronize()
                    there = present(torch, stl, c, ri)
                    assert not (there & ~rb).any(), k
                    good = c.signed_blob_verify_batch_device(*b.dev, tx_ids=True)
                    torch.cuda.synchronize()
                    assert np.array_equal(stl.words_to_bool(good["words"], b.n), rb), k
                    assert np.array_equal(good["status"].cpu().numpy(), rs)
                    assert good["hits"] + good["verified"] == int((rs == stl.TX_OK).sum())
                    continue
                torch.cuda.synchronize()
                assert np.array_equal(stl.words_to_bool(out["words"], b.n), rb)
                assert out["hits"] == want_hits
                break  # no call left to fail
        finally:
            stl.debug_fault_after(-1)
    torch.cuda.synchronize()
    # the blob pass, memset, probe, copy, event, wait, gather, the per-signature launch, scatter, insert
    assert failed == k - 1 and failed >= 10


# ---- 8. two streams, one cache ----
def test_two_streams_one_cache(stl, torch_cuda, oracle, corpus):
    torch = torch_cuda
    batches = [cycled(stl, torch, oracle, corpus, 4099, start=s) for s in (0, 1000)]
    refs = [uncached(torch, stl, b) for b in batches]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, errs = [[], []], []
    torch.cuda.synchronize()
    with stl.SigCache(16, seed=corpus.seed) as c:
        def worker(s):
            try:
                for _ in range(5):
                    o = c.signed_blob_verify_batch_device(*batches[s].dev, tx_ids=True, stream=streams[s])
                    streams[s].synchronize()
                    outs[s].append((stl.words_to_bool(o["words"], 4099), o["status"].cpu().numpy(),
                                    o["tx_id"].cpu().numpy(), o["hits"], o["verified"]))
            except Exception as e:  # noqa: BLE001 - reported below
                errs.append(e)

        ts = [threading.Thread(target=worker, args=(s,)) for s in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        torch.cuda.synchronize()
        assert not errs, errs
        for s in range(2):
            rb, rs, ri, _ = refs[s]
            assert np.array_equal(rb, batches[s].exp)
            assert len(outs[s]) == 5
            for bits, status, ids, hits, verified in outs[s]:
                assert np.array_equal(bits, rb) and np.array_equal(status, rs) and np.array_equal(ids, ri), s
                assert hits + verified == int((rs == stl.TX_OK).sum()) and hits <= int(rb.sum())
            assert outs[s][-1][3] > 0
        # afterwards: what is present was accepted
        # (the IDs as the device gives them: a deferred row's is zero, where the oracle's may be the ID of
        # the accepted blob it was cut from)
        _, _, dev_ids, _ = uncached(torch, stl, corpus)
        there = present(torch, stl, c, dev_ids)
        assert not (there & ~corpus.exp).any() and there.any()


# ---- 9. lifecycle ----
def test_lifecycle_info_host_form_and_stats(stl, torch_cuda, oracle, corpus):
    from stellard_amd import _native as N
    torch = torch_cuda
    lib = N.load()
    b = cycled(stl, torch, oracle, corpus, 600, start=40)
    c = stl.SigCache(10, policy=N.STL_POLICY_SODIUM_1_0_18, seed=0xC0FFEE)
    info = c.info()
    assert info == dict(sets_log2=10, ways=4, kind=stl.BLOB_TRANSACTION, predicate=0,
                        device=torch.cuda.current_device(), bytes=128 << 10, seed=0xC0FFEE)
    with stl.SigCache(3, kind=stl.BLOB_VALIDATION, policy=N.STL_POLICY_STELLARD_1_0_0) as r:
        i2 = r.info()
        assert i2["seed"] != 0 and i2["bytes"] == 128 << 3 and i2["predicate"] == 1 and i2["kind"] == 1
    bits, status, ids, hits, verified = check(torch, stl, c, b)
    ok = status == stl.TX_OK
    assert hits == 0
    _, _, _, hits, _ = check(torch, stl, c, b)
    assert hits > 100
    # clear, then a synchronize: nothing is present
    c.clear()
    torch.cuda.synchronize()
    assert not present(torch, stl, c, ids).any()
    _, _, _, hits, verified = check(torch, stl, c, b)
    assert hits == 0 and verified == int(ok.sum())
    # the host form: the device form's outputs, each row counted once
    stl.reset_stats()
    hb, hs, hi, hhits, hver = c.signed_blob_verify_batch(b.blobs, ids=True)
    st = stl.get_stats()
    assert np.array_equal(hb, bits) and np.array_equal(hs, status)
    assert np.array_equal(hi[ok], ids[ok])
    assert hhits > 100 and hhits + hver == int(ok.sum())
    assert st["signatures"] == b.n and st["batches"] == 1 and st["accepted"] == int(bits.sum())
    c.clear()
    torch.cuda.synchronize()
    stl.reset_stats()
    hb, _, _, hhits, hver = c.signed_blob_verify_batch(b.blobs)
    st = stl.get_stats()
    assert np.array_equal(hb, bits) and (hhits, hver) == (0, int(ok.sum()))
    assert st["signatures"] == b.n and st["batches"] == 1 and st["accepted"] == int(bits.sum())
    # n == 0, then a destroyed handle
    h = c.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    w = torch.zeros(16, dtype=torch.int64, device="cuda")
    s8 = torch.zeros(600, dtype=torch.uint8, device="cuda")
    args = (p(b.dev[0]), p(b.dev[1]), p(b.dev[2]))
    assert lib.stl_sigcache_signed_blob_verify_batch_device(h, *args, 0, p(w), p(s8), None, 0, None, None,
                                                            None) == N.STL_OK
    c.close()
    assert lib.stl_sigcache_signed_blob_verify_batch_device(h, *args, b.n, p(w), p(s8), None, 0, None, None,
                                                            None) == N.STL_EINVAL
    assert lib.stl_sigcache_lookup_device(h, p(s8), 1, p(w), None) == N.STL_EINVAL
    assert lib.stl_sigcache_clear(h, None) == N.STL_EINVAL
    i = stl.SigCacheInfo(struct_size=ctypes.sizeof(stl.SigCacheInfo))
    assert lib.stl_sigcache_get_info(h, ctypes.byref(i)) == N.STL_EINVAL
    lib.stl_sigcache_destroy(h)  # ignored
    with pytest.raises(N.StlError) as e:
        stl.SigCache(25)
    assert e.value.rc == N.STL_EINVAL
