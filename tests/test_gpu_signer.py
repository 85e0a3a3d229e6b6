"""Signer authority on the device: account_id_kernel and tx_signer_kernel
(stellard_amd/csrc/stl_signer.hip) through the C ABI and the Python wrappers.

  * account IDs against OpenSSL's digests (tests/golden/hash160_vectors.json)
    at the wave and workgroup edges, with the bytes past the output intact,
  * the signer pass on 2,000 distinct blobs of every class of
    tests/signer_cases.py, packed back to back, against the Python expectation
    and the host build of the same per-row function,
  * consistency with tx_blob_prepare_device's status and key on the same rows,
  * the one-call blob verify gives the same answer before and after,
  * fault injection on each of the four entry points,
  * the two device calls on two caller streams at once."""
import hashlib

import numpy as np
import pytest

from tests import signer_cases as SC

pytestmark = pytest.mark.gpu

NBLOBS = 2000


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
def keyset():
    """The fixture's keys (m, 32) and their Hash160 by OpenSSL (m, 20)."""
    v = SC.load_vectors()
    keys = np.frombuffer(b"".join(bytes.fromhex(k) for k in v["keys"]), np.uint8).reshape(-1, 32).copy()
    ids = np.frombuffer(b"".join(bytes.fromhex(h) for h in v["hash160"]), np.uint8).reshape(-1, 20).copy()
    return keys, ids


class Corpus:
    """NBLOBS distinct blobs packed back to back, with what each must give."""

    def __init__(self, torch):
        self.cases = SC.make_cases(NBLOBS, 0x516E)
        assert len({c.blob for c in self.cases}) == NBLOBS
        lens = np.array([len(c.blob) for c in self.cases], np.int64)
        self.start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        self.len = lens.astype(np.int32)
        assert set(int(s) % 16 for s in self.start) == set(range(16))  # every alignment of a blob start
        self.bytes = np.frombuffer(b"".join(c.blob for c in self.cases), np.uint8).copy()
        self.signer = np.frombuffer(b"".join(c.signer for c in self.cases), np.uint8).reshape(-1, 20)
        self.account = np.frombuffer(b"".join(c.account for c in self.cases), np.uint8).reshape(-1, 20)
        self.authority = np.array([c.authority for c in self.cases], np.uint8)
        self.status = np.array([c.status for c in self.cases], np.uint8)
        self.acct20 = np.array([c.acct_len == 20 for c in self.cases])
        self.d_bytes = torch.from_numpy(self.bytes).cuda()
        assert self.d_bytes.data_ptr() % 16 == 0

    def rows(self, torch, idx):
        off = torch.from_numpy(self.start[idx]).cuda()
        ln = torch.from_numpy(self.len[idx]).cuda()
        return self.d_bytes, off, ln


@pytest.fixture(scope="module")
def corpus(torch_cuda):
    c = Corpus(torch_cuda)
    # the host build of the same per-row function agrees with the expectation, row for row
    emu = SC.load_signer_emu()
    for i, k in enumerate(c.cases):
        assert SC.emu_row(emu, k.blob) == (k.status, k.signer, k.account, k.authority), (i, k.name)
    return c


def _index(n, seed):
    """n row numbers of the corpus in shuffled order with repeats."""
    return np.random.default_rng(seed).integers(0, NBLOBS, n)


# ---- 1. account IDs ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 70001])
def test_account_id_batch_device(stl, torch_cuda, keyset, n):
    torch = torch_cuda
    keys, ids = keyset
    idx = np.arange(n) % keys.shape[0]
    d_pk = torch.from_numpy(np.ascontiguousarray(keys[idx])).cuda()
    buf = torch.full((20 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[:20 * n].view(n, 20)
    got = stl.account_id_batch_device(d_pk, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    assert np.array_equal(host[:20 * n].reshape(n, 20), ids[idx])
    assert np.all(host[20 * n:] == 0xA5)  # nothing past byte 20 n
    assert np.array_equal(stl.account_id_batch(keys[idx]), ids[idx])


def test_masterpassphrase_account_on_the_device(stl, torch_cuda, oracle):
    """RippleAddress_test's fourth known answer (RippleAddress.cpp:824,850)."""
    pk, _ = oracle.keypair(hashlib.sha512(b"masterpassphrase").digest()[:32])
    d_pk = torch_cuda.from_numpy(np.frombuffer(pk, np.uint8).reshape(1, 32).copy()).cuda()
    got = stl.account_id_batch_device(d_pk).cpu().numpy().tobytes()
    assert got.hex() == "37b1b26be3c91c55d51586c3f0e5c4b03e9cea7f"
    assert stl.account_id_batch(np.frombuffer(pk, np.uint8).reshape(1, 32)).tobytes() == got


# ---- 2. the signer pass ----
@pytest.mark.parametrize("n", [1, 64, 65, 1000, 70001])
def test_tx_blob_signer_batch_device(stl, torch_cuda, corpus, n):
    torch = torch_cuda
    idx = _index(n, 100 + n)
    blobs, off, ln = corpus.rows(torch, idx)
    sbuf = torch.full((20 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    abuf = torch.full((20 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ubuf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = stl.tx_blob_signer_batch_device(blobs, off, ln, out_signer_id=sbuf[:20 * n].view(n, 20),
                                          out_account=abuf[:20 * n].view(n, 20), out_authority=ubuf[:n])
    torch.cuda.synchronize()
    assert np.array_equal(out["authority"].cpu().numpy(), corpus.authority[idx])
    assert np.array_equal(out["signer_id"].cpu().numpy(), corpus.signer[idx])
    assert np.array_equal(out["account"].cpu().numpy(), corpus.account[idx])
    for b, used in ((sbuf, 20 * n), (abuf, 20 * n), (ubuf, n)):
        assert bool((b[used:] == 0xA5).all())
    # without the accounts
    out2 = stl.tx_blob_signer_batch_device(blobs, off, ln, accounts=False)
    torch.cuda.synchronize()
    assert out2["account"] is None
    assert np.array_equal(out2["authority"].cpu().numpy(), corpus.authority[idx])
    assert np.array_equal(out2["signer_id"].cpu().numpy(), corpus.signer[idx])


def test_tx_blob_signer_batch_host_form(stl, corpus):
    idx = _index(300, 7)
    blobs = [corpus.cases[i].blob for i in idx]
    signer, account, authority = stl.tx_blob_signer_batch(blobs)
    assert np.array_equal(authority, corpus.authority[idx])
    assert np.array_equal(signer, corpus.signer[idx])
    assert np.array_equal(account, corpus.account[idx])
    signer2, none, authority2 = stl.tx_blob_signer_batch(blobs, accounts=False)
    assert none is None and np.array_equal(signer2, signer) and np.array_equal(authority2, authority)


def test_every_class_reaches_the_device(corpus):
    idx = _index(1000, 100 + 1000)
    assert {corpus.cases[i].name for i in idx} == set(SC.CLASSES)
    assert set(corpus.authority[idx]) == {SC.NOT_MASTER, SC.MASTER, SC.UNDECIDED}


# ---- 3. consistency with the existing blob pass ----
def test_consistent_with_tx_blob_prepare(stl, torch_cuda, corpus):
    torch = torch_cuda
    idx = np.concatenate([np.arange(NBLOBS), _index(1000, 3)])
    blobs, off, ln = corpus.rows(torch, idx)
    prep = stl.tx_blob_prepare_device(blobs, off, ln)
    out = stl.tx_blob_signer_batch_device(blobs, off, ln)
    ids = stl.account_id_batch_device(prep["pk"])
    torch.cuda.synchronize()
    status = prep["status"].cpu().numpy()
    authority = out["authority"].cpu().numpy()
    assert np.array_equal(status, corpus.status[idx])
    undecided = (status != stl.TX_OK) | ~corpus.acct20[idx]
    assert np.array_equal(authority == stl.SIGNER_UNDECIDED, undecided)
    ok = status == stl.TX_OK
    assert ok.sum() > 1000
    assert np.array_equal(out["signer_id"].cpu().numpy()[ok], ids.cpu().numpy()[ok])
    assert not out["signer_id"].cpu().numpy()[~ok].any()


# ---- 4. the verify path is not disturbed ----
def test_blob_verify_same_before_and_after(stl, torch_cuda, corpus):
    torch = torch_cuda
    idx = _index(3000, 4)
    blobs, off, ln = corpus.rows(torch, idx)

    def verify():
        r = stl.signed_blob_verify_batch_device(blobs, off, ln, tx_ids=True)
        torch.cuda.synchronize()
        return r["words"].cpu().numpy(), r["status"].cpu().numpy(), r["tx_id"].cpu().numpy()

    before = verify()
    out = stl.tx_blob_signer_batch_device(blobs, off, ln)
    after = verify()
    assert np.array_equal(out["authority"].cpu().numpy(), corpus.authority[idx])
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(before[1], corpus.status[idx])


# ---- 5. fault injection ----
def test_fault_injection_every_entry_point(stl, torch_cuda, keyset, corpus):
    from stellard_amd import _native as N
    torch = torch_cuda
    keys, ids = keyset
    idx = _index(500, 5)
    blobs, off, ln = corpus.rows(torch, idx)
    host_blobs = [corpus.cases[i].blob for i in idx]
    d_pk = torch.from_numpy(keys).cuda()
    want_rows = np.concatenate([corpus.signer[idx], corpus.account[idx], corpus.authority[idx][:, None]], axis=1)

    def rows(signer, account, authority):
        return np.concatenate([signer, account, authority[:, None]], axis=1)

    def ids_device():
        out = stl.account_id_batch_device(d_pk)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def signer_device():
        out = stl.tx_blob_signer_batch_device(blobs, off, ln)
        torch.cuda.synchronize()
        return rows(*(out[k].cpu().numpy() for k in ("signer_id", "account", "authority")))

    eps = {
        "account_id_batch": (lambda: stl.account_id_batch(keys), ids),
        "account_id_batch_device": (ids_device, ids),
        "tx_blob_signer_batch": (lambda: rows(*stl.tx_blob_signer_batch(host_blobs)), want_rows),
        "tx_blob_signer_batch_device": (signer_device, want_rows),
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
                    assert np.array_equal(got, exp), (name, k)
                    break
                assert failed < 0, (name, k, failed)
                hits += 1
                assert np.array_equal(call(), exp), (name, k)  # the next clean call is exact
            else:
                pytest.fail(f"{name}: still failing after 40 injected faults")
            report[name] = hits
    finally:
        stl.debug_fault_after(-1)
    assert all(h >= 1 for h in report.values()), report
    assert report["account_id_batch"] >= 4 and report["tx_blob_signer_batch"] >= 8, report


# ---- 6. two caller streams ----
def test_two_streams_concurrently(stl, torch_cuda, keyset, corpus):
    torch = torch_cuda
    keys, ids = keyset
    n = 70001
    kidx = np.random.default_rng(6).integers(0, keys.shape[0], n)
    bidx = _index(n, 66)
    d_pk = torch.from_numpy(np.ascontiguousarray(keys[kidx])).cuda()
    blobs, off, ln = corpus.rows(torch, bidx)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    got_ids, got = [], []
    for _ in range(3):
        got.append(stl.tx_blob_signer_batch_device(blobs, off, ln, stream=s2))
        got_ids.append(stl.account_id_batch_device(d_pk, stream=s1))
    s1.synchronize()
    s2.synchronize()
    for a in got_ids:
        assert np.array_equal(a.cpu().numpy(), ids[kidx])
    for o in got:
        assert np.array_equal(o["authority"].cpu().numpy(), corpus.authority[bidx])
        assert np.array_equal(o["signer_id"].cpu().numpy(), corpus.signer[bidx])
        assert np.array_equal(o["account"].cpu().numpy(), corpus.account[bidx])
