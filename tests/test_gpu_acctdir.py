"""The account directory on the device (stellard_amd/csrc/stl_acctdir.hip)
through the C ABI and the Python wrapper, against the dict model and
Transactor::checkSig as tests/acctdir_py.py restates it.

  * the bare map at the wave and workgroup edges, bytes past the outputs intact,
  * upsert sequences at capacities 1, 5 and 300, and 70,001 accounts at once,
  * 64 IDs that share one home slot, claimed by one wave, wrapped and not,
  * a batch that does not fit is refused and changes nothing,
  * checkSig's verdict on 2,000 blobs of every class of tests/signer_cases.py
    with entries of eight kinds, and the IDs of tx_blob_signer_batch_device,
  * fault injection on every entry point, a re-applied upsert included,
  * the two device calls on two caller streams at once."""
import numpy as np
import pytest

from tests import acctdir_py as AP
from tests import signer_cases as SC

pytestmark = pytest.mark.gpu

NBLOBS = 2000
SAME_HOME_SEED = 0x0123456789ABCDEF


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


def _lookup(torch, d, ids, keys=True, stream=None):
    """(flags, regular keys or None) of the IDs (a list of 20-byte strings) as
    numpy arrays, through lookup_device with guarded outputs."""
    n = len(ids)
    d_ids = torch.from_numpy(AP.id_array(ids)).cuda()
    fbuf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    kbuf = torch.full((20 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = d.lookup_device(d_ids, regular_keys=keys, stream=stream, out_flags=fbuf[:n],
                          out_regular_key=kbuf[:20 * n].view(n, 20) if keys else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert bool((fbuf[n:] == 0xA5).all())  # nothing past byte n
    assert bool((kbuf[20 * n if keys else 0:] == 0xA5).all())  # nothing past byte 20 n, or nothing at all
    assert (out["regular_key"] is None) == (not keys)
    return fbuf[:n].cpu().numpy(), (kbuf[:20 * n].view(n, 20).cpu().numpy() if keys else None)


def _check(torch, d, model, ids):
    f, k = _lookup(torch, d, ids)
    wf, wk = model.lookup_arrays(ids)
    assert np.array_equal(f, wf)
    assert np.array_equal(k, wk)


# ---- 1. the bare map ----
@pytest.fixture(scope="module")
def loaded(stl, torch_cuda):
    """A directory of 3,000 accounts of every flags value (ABSENT ones too),
    its model, the accounts and 1,000 strangers."""
    rng = np.random.default_rng(11)
    ids = [rng.bytes(20) for _ in range(3000)]
    flags = rng.integers(0, 8, 3000).astype(np.uint8)
    keys = [rng.bytes(20) for _ in range(3000)]
    model = AP.Model(4000)
    d = stl.AccountDirectory(4000)
    assert model.upsert(ids, flags, keys)
    d.upsert(AP.id_array(ids), flags, AP.id_array(keys))
    assert d.info()["records"] == 3000
    yield d, model, ids, [rng.bytes(20) for _ in range(1000)]
    d.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 70001])
def test_lookup_device(stl, torch_cuda, loaded, n):
    torch = torch_cuda
    d, model, ids, strangers = loaded
    pool = ids + strangers
    q = [pool[i] for i in np.random.default_rng(n).integers(0, len(pool), n)]
    wf, wk = model.lookup_arrays(q)
    if n >= 255:
        assert {0, 1, 2, 3, AP.NOT_FOUND} == set(wf)
    f, k = _lookup(torch, d, q)
    assert np.array_equal(f, wf) and np.array_equal(k, wk)
    f2, none = _lookup(torch, d, q, keys=False)
    assert none is None and np.array_equal(f2, wf)
    f3, k3 = _lookup(torch, d, q, stream=torch.cuda.Stream())
    assert np.array_equal(f3, wf) and np.array_equal(k3, wk)


# ---- 2. upsert sequences ----
@pytest.mark.parametrize("capacity", [1, 5, 300])
def test_upsert_sequence(stl, torch_cuda, capacity):
    """create -> upsert A -> check -> upsert B, C, D (overlapping what is there:
    changed flags and keys, new IDs, some ABSENT, duplicates inside a batch)
    -> check after each.  A batch's IDs all count against the capacity, so at
    capacity 1 every batch after the first is refused and changes nothing."""
    from stellard_amd import _native as N
    torch = torch_cuda
    rng = np.random.default_rng(200 + capacity)
    model = AP.Model(capacity)
    known, strangers = [], [rng.bytes(20) for _ in range(70)]
    applied = refused = 0
    with stl.AccountDirectory(capacity, seed=77 + capacity) as d:
        info = d.info()
        assert (info["capacity"], info["records"], info["slots"], info["seed"]) == \
            (capacity, 0, AP.slots_for(capacity), 77 + capacity)
        assert info["bytes"] == 4 * info["slots"] + 48 * capacity
        _check(torch, d, model, strangers)
        for _ in range(4):
            ids, flags, keys = AP.random_batch(rng, known, max(1, capacity // 3))
            if model.upsert(ids, flags, keys):
                d.upsert(AP.id_array(ids), flags, AP.id_array(keys))
                applied += 1
            else:
                with pytest.raises(N.StlError) as e:
                    d.upsert(AP.id_array(ids), flags, AP.id_array(keys))
                assert e.value.rc == N.STL_ENOMEM
                refused += 1
            _check(torch, d, model, known + strangers)
            assert d.info()["records"] == len(model.state)
        assert applied >= 1 and (capacity > 1 or refused == 3)


def test_upsert_70001_fresh_accounts(stl, torch_cuda):
    """Many workgroups claim slots at once."""
    torch = torch_cuda
    n = 70001
    rng = np.random.default_rng(70001)
    ids = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    assert len({r.tobytes() for r in ids}) == n
    flags = rng.integers(0, 4, n).astype(np.uint8)
    keys = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    with stl.AccountDirectory(n) as d:
        d.upsert(ids, flags, keys)
        info = d.info()
        assert info["records"] == n and info["slots"] == 1 << 19
        assert 2 <= info["longest_probe"] <= 64  # a load of 0.13: runs stay short
        out = d.lookup_device(torch.from_numpy(ids).cuda())
        miss = d.lookup_device(torch.from_numpy(ids ^ np.uint8(1)).cuda())
        torch.cuda.synchronize()
        assert np.array_equal(out["flags"].cpu().numpy(), flags)
        want_keys = np.where((flags & AP.HAS_REGULAR_KEY)[:, None] != 0, keys, 0)
        assert np.array_equal(out["regular_key"].cpu().numpy(), want_keys)
        assert bool((miss["flags"] == AP.NOT_FOUND).all()) and not bool(miss["regular_key"].any())


# ---- 3. IDs that share a home slot ----
@pytest.mark.parametrize("home", [0, 250])
def test_same_home_ids(stl, torch_cuda, home):
    """64 lanes of one wave contend for one run of slots (from slot 250 of 256
    the run wraps)."""
    torch = torch_cuda
    ids = AP.same_home_ids(64, home, 256, SAME_HOME_SEED, 40 + home)
    rng = np.random.default_rng(home)
    keys = [rng.bytes(20) for _ in ids]
    strangers = [rng.bytes(20) for _ in range(64)]
    model = AP.Model(64)
    flags = np.full(64, AP.HAS_REGULAR_KEY, np.uint8)
    with stl.AccountDirectory(64, seed=SAME_HOME_SEED) as d:
        assert d.info()["slots"] == 256
        model.upsert(ids, flags, keys)
        d.upsert(AP.id_array(ids), flags, AP.id_array(keys))
        assert d.info()["longest_probe"] == 64 and d.info()["records"] == 64
        _check(torch, d, model, ids)
        f, k = _lookup(torch, d, strangers)
        assert np.all(f == AP.NOT_FOUND) and not k.any()


# ---- 4. a batch that does not fit ----
def test_capacity_refusal(stl, torch_cuda):
    from stellard_amd import _native as N
    torch = torch_cuda
    rng = np.random.default_rng(4)
    a = [rng.bytes(20) for _ in range(6)]
    b = [rng.bytes(20) for _ in range(4)] + [a[0]]
    fa, fb = np.full(6, AP.HAS_REGULAR_KEY, np.uint8), np.full(5, AP.MASTER_DISABLED, np.uint8)
    with stl.AccountDirectory(10) as d:
        d.upsert(AP.id_array(a), fa, AP.id_array(a[::-1]))
        before = _lookup(torch, d, a + b)
        with pytest.raises(N.StlError) as e:
            d.upsert(AP.id_array(b), fb)  # 6 + 5 > 10
        assert e.value.rc == N.STL_ENOMEM
        after = _lookup(torch, d, a + b)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert d.info()["records"] == 6
        d.upsert(AP.id_array(b[1:]), fb[1:])  # 6 + 4 fits
        assert d.info()["records"] == 9
        f, _ = _lookup(torch, d, a + b)
        assert list(f) == [AP.MASTER_DISABLED] + [AP.HAS_REGULAR_KEY] * 5 + [AP.NOT_FOUND] + [AP.MASTER_DISABLED] * 4
        with pytest.raises(N.StlError) as e:
            d.upsert(AP.id_array(a[:1]), np.array([0x10], np.uint8))
        assert e.value.rc == N.STL_EINVAL
        with pytest.raises(N.StlError) as e:
            d.upsert(AP.id_array(a[:1]), np.array([AP.HAS_REGULAR_KEY], np.uint8))  # no keys given
        assert e.value.rc == N.STL_EINVAL


# ---- 5. checkSig's verdict ----
class Corpus:
    """NBLOBS distinct blobs packed back to back, the directory entries of
    their accounts, and what each row must give."""

    def __init__(self, torch, stl):
        self.cases = SC.make_cases(NBLOBS, 0xACC7D1)
        assert len({c.blob for c in self.cases}) == NBLOBS
        lens = np.array([len(c.blob) for c in self.cases], np.int64)
        self.start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        self.len = lens.astype(np.int32)
        self.bytes = np.frombuffer(b"".join(c.blob for c in self.cases), np.uint8).copy()
        self.d_bytes = torch.from_numpy(self.bytes).cuda()
        self.ids, self.flags, self.keys, self.want, self.model = AP.corpus_entries(self.cases, 55)
        self.dir = stl.AccountDirectory(len(self.ids) + 64)
        self.dir.upsert(AP.id_array(self.ids), self.flags, AP.id_array(self.keys))

    def rows(self, torch, idx):
        return (self.d_bytes, torch.from_numpy(self.start[idx]).cuda(), torch.from_numpy(self.len[idx]).cuda())


@pytest.fixture(scope="module")
def corpus(torch_cuda, stl):
    c = Corpus(torch_cuda, stl)
    yield c
    c.dir.close()


def _index(n, seed):
    return np.random.default_rng(seed).integers(0, NBLOBS, n)


def test_corpus_reaches_every_verdict(corpus):
    counts = np.bincount(corpus.want, minlength=7)
    assert len(counts) == 7 and counts.min() >= 20, counts
    assert {c.name for c in corpus.cases} == set(SC.CLASSES)
    # the master branch first: master-signed, MASTER_DISABLED, RegularKey == Account
    hits = [i for i, c in enumerate(corpus.cases)
            if c.authority == SC.MASTER and
            corpus.model.state.get(c.account, (0, b"")) == (AP.HAS_REGULAR_KEY | AP.MASTER_DISABLED, c.account)]
    assert len(hits) >= 20 and all(corpus.want[i] == AP.AUTH_MASTER_DISABLED for i in hits)


@pytest.mark.parametrize("n", [1, 64, 65, 1000, 70001])
def test_tx_blob_authority_device(stl, torch_cuda, corpus, n):
    torch = torch_cuda
    idx = _index(n, 500 + n)
    blobs, off, ln = corpus.rows(torch, idx)
    ref = stl.tx_blob_signer_batch_device(blobs, off, ln)
    torch.cuda.synchronize()
    ref_signer, ref_account = ref["signer_id"].cpu().numpy(), ref["account"].cpu().numpy()
    want = corpus.want[idx]
    if n >= 1000:
        assert set(want) == set(range(7))
    for with_signer, with_account in ((True, True), (True, False), (False, True), (False, False)):
        sbuf = torch.full((20 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        abuf = torch.full((20 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        ubuf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out = corpus.dir.tx_blob_authority_device(
            blobs, off, ln, signer_ids=with_signer, accounts=with_account,
            out_signer_id=sbuf[:20 * n].view(n, 20) if with_signer else None,
            out_account=abuf[:20 * n].view(n, 20) if with_account else None, out_authority=ubuf[:n])
        torch.cuda.synchronize()
        assert np.array_equal(out["authority"].cpu().numpy(), want)
        assert (out["signer_id"] is None) == (not with_signer) and (out["account"] is None) == (not with_account)
        if with_signer:
            assert np.array_equal(out["signer_id"].cpu().numpy(), ref_signer)  # bit for bit
        if with_account:
            assert np.array_equal(out["account"].cpu().numpy(), ref_account)
        assert bool((sbuf[20 * n if with_signer else 0:] == 0xA5).all())
        assert bool((abuf[20 * n if with_account else 0:] == 0xA5).all())
        assert bool((ubuf[n:] == 0xA5).all())


def test_tx_blob_authority_host_form(stl, corpus):
    idx = _index(300, 7)
    blobs = [corpus.cases[i].blob for i in idx]
    signer, account, authority = corpus.dir.tx_blob_authority(blobs)
    assert np.array_equal(authority, corpus.want[idx])
    assert np.array_equal(signer, np.frombuffer(b"".join(corpus.cases[i].signer for i in idx), np.uint8).reshape(-1, 20))
    assert np.array_equal(account,
                          np.frombuffer(b"".join(corpus.cases[i].account for i in idx), np.uint8).reshape(-1, 20))
    s2, a2, authority2 = corpus.dir.tx_blob_authority(blobs, signer_ids=False, accounts=False)
    assert s2 is None and a2 is None and np.array_equal(authority2, authority)
    ref_signer, ref_account, _ = stl.tx_blob_signer_batch(blobs)
    assert np.array_equal(signer, ref_signer) and np.array_equal(account, ref_account)


def test_verdict_follows_the_snapshot(stl, torch_cuda):
    """The same rows, before and after an upsert that changes their accounts."""
    torch = torch_cuda
    cases = [c for c in SC.make_cases(64, 0x51AB) if c.authority != SC.UNDECIDED]
    blob = np.frombuffer(b"".join(c.blob for c in cases), np.uint8).copy()
    lens = np.array([len(c.blob) for c in cases], np.int64)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).cuda()
    ln = torch.from_numpy(lens.astype(np.int32)).cuda()
    d_blob = torch.from_numpy(blob).cuda()
    ids = AP.id_array([c.account for c in cases])
    with stl.AccountDirectory(2 * len(cases)) as d:  # room for a batch that names every account again
        def verdicts():
            out = d.tx_blob_authority_device(d_blob, off, ln)
            torch.cuda.synchronize()
            return list(out["authority"].cpu().numpy())

        def expect(entry_of):
            return [AP.check_sig(c.signer, c.account, entry_of(c)) for c in cases]

        assert verdicts() == expect(lambda c: None)
        d.upsert(ids, np.zeros(len(cases), np.uint8))
        assert verdicts() == expect(lambda c: AP.Entry())
        d.upsert(ids, np.full(len(cases), AP.HAS_REGULAR_KEY | AP.MASTER_DISABLED, np.uint8),
                 AP.id_array([c.signer for c in cases]))
        assert verdicts() == expect(lambda c: AP.Entry(c.signer, True))
        d.upsert(ids, np.full(len(cases), AP.ABSENT, np.uint8))
        assert verdicts() == expect(lambda c: None)
        assert d.info()["records"] == len(cases)


# ---- 6. fault injection ----
def test_fault_injection_every_entry_point(stl, torch_cuda, corpus):
    """stl_debug_fault_after: a host-side countdown that skips one HIP call of
    the library and reports its failure (nothing faults on the device)."""
    from stellard_amd import _native as N
    torch = torch_cuda
    idx = _index(500, 5)
    blobs, off, ln = corpus.rows(torch, idx)
    host_blobs = [corpus.cases[i].blob for i in idx]
    ref = stl.tx_blob_signer_batch_device(blobs, off, ln)
    torch.cuda.synchronize()
    want_rows = np.concatenate([ref["signer_id"].cpu().numpy(), ref["account"].cpu().numpy(),
                                corpus.want[idx][:, None]], axis=1)
    q = corpus.ids[:400] + [bytes([i]) * 20 for i in range(100)]
    d_q = torch.from_numpy(AP.id_array(q)).cuda()
    wf, wk = corpus.model.lookup_arrays(q)
    want_lookup = np.concatenate([wf[:, None], wk], axis=1)

    def authority_device():
        out = corpus.dir.tx_blob_authority_device(blobs, off, ln)
        torch.cuda.synchronize()
        return np.concatenate([out[k].cpu().numpy() for k in ("signer_id", "account")] +
                              [out["authority"].cpu().numpy()[:, None]], axis=1)

    def authority_host():
        s, a, u = corpus.dir.tx_blob_authority(host_blobs)
        return np.concatenate([s, a, u[:, None]], axis=1)

    def lookup_device():
        out = corpus.dir.lookup_device(d_q)
        torch.cuda.synchronize()
        return np.concatenate([out["flags"].cpu().numpy()[:, None], out["regular_key"].cpu().numpy()], axis=1)

    def create():
        with stl.AccountDirectory(5, seed=9) as d:
            return np.array([d.info()[k] for k in ("capacity", "records", "slots", "longest_probe")])

    # upsert: every attempt is a new batch on one directory, checked against the model
    rng = np.random.default_rng(66)
    up_model, up_known = AP.Model(1 << 20), []
    up_dir = stl.AccountDirectory(8192)

    def upsert():
        ids, flags, keys = AP.random_batch(rng, up_known, 60)
        try:
            up_dir.upsert(AP.id_array(ids), flags, AP.id_array(keys))
        except N.StlError:
            # may have applied any part of the batch: applying it again completes it
            stl.debug_fault_after(-1)
            up_model.upsert(ids, flags, keys)
            up_dir.upsert(AP.id_array(ids), flags, AP.id_array(keys))
            _check(torch, up_dir, up_model, up_known)
            assert len(up_model.state) <= up_dir.info()["records"] <= 8192
            raise
        up_model.upsert(ids, flags, keys)
        f, k = _lookup(torch, up_dir, up_known)
        return np.concatenate([f[:, None], k], axis=1)

    def upsert_expected():
        wf2, wk2 = up_model.lookup_arrays(up_known)
        return np.concatenate([wf2[:, None], wk2], axis=1)

    eps = {
        "acctdir_create": (create, lambda: np.array([5, 0, 32, 0])),
        "acctdir_upsert": (upsert, upsert_expected),
        "acctdir_lookup_device": (lookup_device, lambda: want_lookup),
        "acctdir_tx_blob_authority_device": (authority_device, lambda: want_rows),
        "acctdir_tx_blob_authority": (authority_host, lambda: want_rows),
    }
    report = {}
    try:
        for name, (call, exp) in eps.items():
            hits = 0
            for k in range(0, 40):
                stl.debug_fault_after(k)
                try:
                    got = call()
                    failed = None
                except N.StlError as e:
                    failed = e.rc
                stl.debug_fault_after(-1)
                if failed is None:
                    # the countdown outlived the call: a clean, exact result
                    assert np.array_equal(got, exp()), (name, k)
                    break
                assert failed < 0, (name, k, failed)
                hits += 1
                assert np.array_equal(call(), exp()), (name, k)  # the next clean call is exact
            else:
                pytest.fail(f"{name}: still failing after 40 injected faults")
            report[name] = hits
    finally:
        stl.debug_fault_after(-1)
        up_dir.close()
    assert all(h >= 1 for h in report.values()), report
    assert report["acctdir_upsert"] >= 4 and report["acctdir_tx_blob_authority"] >= 8, report
    assert report["acctdir_create"] >= 6, report


# ---- 7. two caller streams ----
def test_two_streams_concurrently(stl, torch_cuda, corpus):
    torch = torch_cuda
    n = 70001
    bidx = _index(n, 66)
    blobs, off, ln = corpus.rows(torch, bidx)
    pool = corpus.ids + [bytes([i]) * 20 for i in range(200)]
    q = [pool[i] for i in np.random.default_rng(67).integers(0, len(pool), n)]
    d_q = torch.from_numpy(AP.id_array(q)).cuda()
    wf, wk = corpus.model.lookup_arrays(q)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    got_l, got_a = [], []
    for _ in range(3):
        got_a.append(corpus.dir.tx_blob_authority_device(blobs, off, ln, stream=s2))
        got_l.append(corpus.dir.lookup_device(d_q, stream=s1))
    s1.synchronize()
    s2.synchronize()
    for o in got_l:
        assert np.array_equal(o["flags"].cpu().numpy(), wf) and np.array_equal(o["regular_key"].cpu().numpy(), wk)
    for o in got_a:
        assert np.array_equal(o["authority"].cpu().numpy(), corpus.want[bidx])
