"""GPU tests of the SHAMap root (stl_shamap_root*): the root and the four
counts of every call equal the model of tests/shamap_py.py, on guarded output
buffers -- the 32 root bytes and the 16 count bytes are written and nothing
beside them.

Run on an MI355X:  python -u -m pytest tests/test_gpu_shamap.py -m gpu -x -v
"""
import hashlib
import json
import threading

import numpy as np
import pytest

from tests import shamap_py as SM
from tests import txblob

pytestmark = pytest.mark.gpu

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


def words_of(torch, select):
    """bool[n] -> the int64 bitmap words of the accept bitmaps' layout, on the device."""
    n = len(select)
    packed = np.packbits(np.asarray(select, dtype=bool), bitorder="little")
    buf = np.zeros((n + 63) // 64 * 8, np.uint8)
    buf[:packed.size] = packed
    return torch.from_numpy(buf.view(np.int64).copy()).cuda()


def run(torch, stl, keys, leaves=None, select=None, stream=None, words=None):
    """One device call on guarded buffers -> (root bytes, counts list)."""
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    k, lh = dev(keys), dev(leaves)
    if k is None or k.shape[0] == 0:
        k = torch.zeros((0, 32), dtype=torch.uint8, device="cuda")
    w = words if words is not None else (None if select is None else words_of(torch, select))
    root = torch.full((3, 32), GUARD, dtype=torch.uint8, device="cuda")
    cnt = torch.full((12,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stl.shamap_root_device(k, lh, w, out_root=root[1:2], counts=cnt[4:8], stream=stream)
    torch.cuda.synchronize()
    assert (root[0] == GUARD).all() and (root[2] == GUARD).all(), "guard bytes beside the root overwritten"
    assert (cnt[:4] == 0x5A5A5A5A).all() and (cnt[8:] == 0x5A5A5A5A).all(), "guard words beside the counts overwritten"
    return root[1].cpu().numpy().tobytes(), [int(x) for x in cnt[4:8].cpu().numpy()]


def check(torch, stl, keys, leaves=None, select=None, stream=None):
    want = SM.model(keys, leaves, select)
    got = run(torch, stl, keys, leaves, select, stream)
    assert got[1] == want[1], (got[1], want[1])
    assert got[0] == want[0]
    return got


def _leaves(keys, seed):
    return np.random.default_rng(seed).integers(0, 256, keys.shape, dtype=np.uint8)


# ---- 1. the shapes ----
def test_golden_roots(stl, torch_cuda):
    """The committed fixture: every case's root and counts, from the device."""
    with open(SM.GOLDEN) as f:
        doc = json.load(f)
    for c in doc["cases"]:
        root, counts = run(torch_cuda, stl, SM.case_keys(c["shape"], c["seed"]))
        assert (root.hex(), counts) == (c["root"], c["counts"]), c["shape"]


def test_tiny_maps(stl, torch_cuda):
    torch = torch_cuda
    assert run(torch, stl, np.zeros((0, 32), np.uint8)) == (SM.ZERO, [0, 0, 0, 0])
    for shape in ("random1", "random2", "root17"):
        check(torch, stl, SM.case_keys(shape, 41))
    # one item: its leaf under the root, whatever its leaf hash
    k = SM.case_keys("random1", 42)
    lh = _leaves(k, 43)
    root, _ = check(torch, stl, k, lh)
    b = k[0, 0] >> 4
    assert root == SM.inner_hash([lh[0].tobytes() if i == b else SM.ZERO for i in range(16)])


def test_deepest_chain_and_dense_deep_subtree(stl, torch_cuda):
    _, c = check(torch_cuda, stl, SM.case_keys("deepest", 44))
    assert c == [2, 0, 64, 63]
    _, c = check(torch_cuda, stl, SM.case_keys("dense", 45))
    assert c[0] == 4096 and c[3] == 63 and c[2] > 60 + 256
    check(torch_cuda, stl, SM.case_keys("cluster3000_5_62", 46))


def test_multi_word_sort(stl, torch_cuda):
    """Keys equal in their first 8, 16 and 24 bytes among random ones: the
    sort has to be exact past the first words."""
    keys = SM.case_keys("multiword", 47)
    check(torch_cuda, stl, keys)
    big = np.concatenate([SM.case_keys("random3000", 48), keys, SM.case_keys("cluster900_4_16", 49),
                          SM.case_keys("cluster900_4_32", 50), SM.case_keys("cluster900_4_48", 51)])
    check(torch_cuda, stl, big[np.random.default_rng(52).permutation(big.shape[0])], _leaves(big, 53))


@pytest.mark.parametrize("n", [63, 64, 65, 255, 257, 4097, 65537, 131073])
def test_random_keys(stl, torch_cuda, n):
    check(torch_cuda, stl, SM.case_keys(f"random{n}", n))


# ---- 2. set semantics, leaf hashes, the select bitmap ----
def test_set_semantics(stl, torch_cuda):
    torch = torch_cuda
    keys = SM.case_keys("random5000", 60)
    root, c = check(torch, stl, keys)
    rng = np.random.default_rng(61)
    assert run(torch, stl, keys[rng.permutation(5000)]) == (root, c)
    dup = np.concatenate([keys, keys[rng.integers(0, 5000, 777)]])
    dup = dup[rng.permutation(dup.shape[0])]
    assert run(torch, stl, dup) == (root, [5000, 777, c[2], c[3]])
    check(torch, stl, SM.case_keys("dups4097", 62))
    # one key, many times over
    _, c1 = check(torch, stl, np.repeat(keys[:1], 1000, axis=0))
    assert c1 == [1, 999, 1, 0]


def test_leaf_hashes(stl, torch_cuda):
    torch = torch_cuda
    keys = SM.case_keys("random4097", 63)
    lh = _leaves(keys, 64)
    with_leaves, _ = check(torch, stl, keys, lh)
    assert with_leaves != check(torch, stl, keys)[0]
    assert run(torch, stl, keys, keys)[0] == SM.model(keys)[0]  # leaf hash = key, given explicitly
    # duplicate keys with different leaf hashes: the lowest selected row wins
    k2 = np.concatenate([keys[:600], keys[:600], keys[:600]])
    l2 = _leaves(k2, 65)
    root, c = check(torch, stl, k2, l2)
    assert c[:2] == [600, 1200] and root == SM.model(keys[:600], l2[:600])[0]
    sel = np.ones(1800, bool)
    sel[:600:2] = False  # every other first copy is off: its second copy supplies the hash
    root, _ = check(torch, stl, k2, l2, sel)
    mixed = l2[:600].copy()
    mixed[::2] = l2[600:1200:2]
    assert root == SM.model(keys[:600], mixed)[0]


def test_select_bitmap(stl, torch_cuda):
    torch = torch_cuda
    for n in (65, 1000, 4097):
        keys = SM.case_keys(f"dups{n}", 66 + n)
        lh = _leaves(keys, 67)
        root, c = check(torch, stl, keys, lh)
        assert run(torch, stl, keys, lh, np.ones(n, bool)) == (root, c)
        # bits past n in the last word are ignored
        w = words_of(torch, np.ones(n, bool))
        w[-1] = -1
        assert run(torch, stl, keys, lh, words=w) == (root, c)
        assert run(torch, stl, keys, lh, np.zeros(n, bool)) == (SM.ZERO, [0, 0, 0, 0])
        sel = np.random.default_rng(68 + n).random(n) < 0.5
        got = check(torch, stl, keys, lh, sel)
        sub = np.nonzero(sel)[0]
        assert got == SM.model(keys[sub], lh[sub])
        one = np.zeros(n, bool)
        one[n - 1] = True
        check(torch, stl, keys, lh, one)


# ---- 3. from blobs and from the verify's bitmap ----
def test_from_blobs_and_accept_words(stl, torch_cuda, oracle):
    """The IDs the blob call writes give the root of the model over
    SHA512Half("TXN\\0" || blob); its accept words select the accepted rows."""
    from stellard_amd.verify import _pack
    torch = torch_cuda
    rng = np.random.default_rng(70)
    good = txblob.valid_corpus(oracle, 300, 71)
    blobs = list(good)
    for i in range(0, 300, 5):  # a flipped signature bit: the ID stands, the verify rejects
        b = bytearray(blobs[i])
        at = blobs[i].find(b"\x74\x40") + 2 + int(rng.integers(0, 64))
        b[at] ^= 1
        blobs[i] = bytes(b)
    blobs += blobs[:20]  # repeats: dropped as duplicates
    buf, offs, lens = _pack(blobs)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (buf, offs.view(np.int64), lens.view(np.int32))]
    out = stl.signed_blob_verify_batch_device(*dev, tx_ids=True)
    torch.cuda.synchronize()
    n = len(blobs)
    assert (out["status"].cpu().numpy() == stl.TX_OK).all()
    ids = np.stack([np.frombuffer(hashlib.sha512(b"TXN\0" + b).digest()[:32], np.uint8) for b in blobs])
    assert np.array_equal(out["tx_id"].cpu().numpy(), ids)
    want = SM.model(ids)
    assert want[1][:2] == [300, 20]
    for stream in (None, torch.cuda.Stream()):
        root = torch.full((3, 32), GUARD, dtype=torch.uint8, device="cuda")
        cnt = torch.full((6,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        stl.shamap_root_device(out["tx_id"], out_root=root[1:2], counts=cnt[1:5], stream=stream)
        torch.cuda.synchronize()
        assert (root[1].cpu().numpy().tobytes(), [int(x) for x in cnt[1:5].cpu().numpy()]) == want
        assert (root[::2] == GUARD).all() and int(cnt[0]) == 7 and int(cnt[5]) == 7
    # the verify's own accept words
    bits = stl.words_to_bool(out["words"], n)
    assert 200 < int(bits.sum()) < n
    accepted = run(torch, stl, ids, words=out["words"])
    assert accepted == SM.model(ids, None, bits) == SM.model(ids[np.nonzero(bits)[0]])
    assert accepted[0] != want[0]
    # the host form on the same IDs
    assert stl.shamap_root(ids, counts=True) == want
    assert stl.shamap_root(ids, select=bits, counts=True) == accepted
    lh = _leaves(ids, 72)
    assert stl.shamap_root(ids, leaf_hashes=lh, select=bits, counts=True) == SM.model(ids, lh, bits)
    assert stl.shamap_root(np.zeros((0, 32), np.uint8), counts=True) == (SM.ZERO, [0, 0, 0, 0])
    assert stl.shamap_root(ids[:1]) == SM.model(ids[:1])[0]


# ---- 4. streams ----
def test_streams(stl, torch_cuda):
    torch = torch_cuda
    a, b = SM.case_keys("random4097", 80), SM.case_keys("cluster3000_9_20", 81)
    la = _leaves(a, 82)
    want_a, want_b = SM.model(a, la), SM.model(b)
    s = torch.cuda.Stream()
    # a non-default stream, twice in a row with different sizes: the second reuses the workspace
    # behind the first in stream order, with no wait between them
    ka, kb, lda = (torch.from_numpy(x).cuda() for x in (a, b, la))
    torch.cuda.synchronize()
    ra, ca = stl.shamap_root_device(ka, lda, counts=True, stream=s)
    rb, cb = stl.shamap_root_device(kb, counts=True, stream=s)
    ra2 = stl.shamap_root_device(ka, lda, stream=s)
    torch.cuda.synchronize()
    assert (ra.cpu().numpy().tobytes(), [int(x) for x in ca.cpu()]) == want_a
    assert (rb.cpu().numpy().tobytes(), [int(x) for x in cb.cpu()]) == want_b
    assert ra2.cpu().numpy().tobytes() == want_a[0]
    # two streams at once, from two threads
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    errs = []

    def worker(i):
        try:
            keys, lh, want = (a, la, want_a) if i == 0 else (b, None, want_b)
            for _ in range(4):
                assert run(torch, stl, keys, lh, stream=streams[i]) == want
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errs.append(e)

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


# ---- 5. injected errors ----
def test_fault_injection(stl, torch_cuda):
    """Every HIP call of one device call and of one host call failed in turn:
    the call returns < 0 and leaves its outputs alone, and the next clean call
    is right."""
    from stellard_amd import _native as N
    torch = torch_cuda
    keys = SM.case_keys("dups1000", 90)
    lh = _leaves(keys, 91)
    sel = np.random.default_rng(92).random(1000) < 0.7
    want = SM.model(keys, lh, sel)
    k, l, w = torch.from_numpy(keys).cuda(), torch.from_numpy(lh).cuda(), words_of(torch, sel)
    stream = torch.cuda.Stream()  # a fresh context: the first call also allocates
    for form in ("device", "host"):
        failed, kk = 0, 0
        try:
            while True:
                assert kk < 200, "the countdown never ran out"
                root = torch.full((1, 32), GUARD, dtype=torch.uint8, device="cuda")
                cnt = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                stl.debug_fault_after(kk)
                kk += 1
                try:
                    if form == "device":
                        stl.shamap_root_device(k, l, w, out_root=root, counts=cnt, stream=stream)
                        torch.cuda.synchronize()
                        got = (root[0].cpu().numpy().tobytes(), [int(x) for x in cnt.cpu().numpy()])
                    else:
                        got = stl.shamap_root(keys, lh, sel, counts=True)
                except N.StlError as e:
                    assert e.rc < 0
                    failed += 1
                    stl.debug_fault_after(-1)
                    torch.cuda.synchronize()
                    # never a root: the outputs are the last launch's alone
                    assert (root == GUARD).all() and (cnt == 0x5A5A5A5A).all(), kk
                    assert run(torch, stl, keys, lh, sel, stream=stream) == want, kk
                    continue
                assert got == want
                break  # no call left to fail
        finally:
            stl.debug_fault_after(-1)
        torch.cuda.synchronize()
        # the workspace, the memset, 4 + 1 word kernels and sorts, heads, scan, compact, neighbours, 64 levels, finish
        assert failed == kk - 1 and failed >= 80, (form, failed)
