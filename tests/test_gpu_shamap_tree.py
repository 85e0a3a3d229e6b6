"""GPU tests of the resident SHAMap (stl_shamap_tree_*): after every apply the
root and the eight counts equal the model of tests/shamap_tree_py.py and the
exported content equals the model's sorted dict, on guarded buffers -- the 32
root bytes, the 32 count bytes and the exported rows are written and nothing
beside them.

Run on an MI355X:  python -u -m pytest tests/test_gpu_shamap_tree.py -m gpu -x -v
"""
import ctypes
import json

import numpy as np
import pytest

from tests import shamap_py as SM
from tests import shamap_tree_py as TM

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_WORD = 0x5A5A5A5A


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


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def apply_guarded(torch, tree, keys, leaves=None, ops=None, stream=None):
    """One device apply on guarded outputs -> (root bytes, counts list)."""
    k, lh, op = _dev(torch, keys), _dev(torch, leaves), _dev(torch, ops)
    if k.shape[0] == 0:
        k = torch.zeros((0, 32), dtype=torch.uint8, device="cuda")
    root = torch.full((3, 32), GUARD, dtype=torch.uint8, device="cuda")
    cnt = torch.full((24,), GUARD_WORD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tree.apply_device(k, lh, op, out_root=root[1:2], counts=cnt[8:16], stream=stream)
    torch.cuda.synchronize()
    assert (root[0] == GUARD).all() and (root[2] == GUARD).all(), "guard bytes beside the root overwritten"
    assert (cnt[:8] == GUARD_WORD).all() and (cnt[16:] == GUARD_WORD).all(), "guard words beside the counts overwritten"
    return root[1].cpu().numpy().tobytes(), [int(x) for x in cnt[8:16].cpu().numpy()]


def exported(torch, tree, rows, stream=None):
    """The tree's content through export_device on guarded buffers -> (keys, leaves) as device tensors."""
    k = torch.full((rows + 2, 32), GUARD, dtype=torch.uint8, device="cuda")
    l = torch.full((rows + 2, 32), GUARD, dtype=torch.uint8, device="cuda")
    items = torch.full((3,), GUARD_WORD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tree.export_device(k[1:rows + 1], l[1:rows + 1], items[1:2], stream=stream)
    torch.cuda.synchronize()
    m = int(items[1])
    assert int(items[0]) == GUARD_WORD and int(items[2]) == GUARD_WORD
    assert 0 <= m <= rows
    for t in (k, l):
        assert (t[0] == GUARD).all() and (t[m + 1:] == GUARD).all(), "rows beside the content overwritten"
    return k[1:m + 1], l[1:m + 1]


class Rig:
    """A tree on the device and its model, stepped together."""

    def __init__(self, torch, stl, capacity, stream=None):
        self.torch, self.stl, self.cap, self.stream = torch, stl, capacity, stream
        self.tree = stl.ShamapTree(capacity)
        self.m = TM.Model()

    def check_content(self, want_root, against_root_call=False):
        torch = self.torch
        k, l = exported(torch, self.tree, self.cap, self.stream)
        wk, wl = self.m.content()
        assert k.shape[0] == wk.shape[0]
        assert np.array_equal(k.cpu().numpy(), wk), "exported keys differ from the sorted dict"
        assert np.array_equal(l.cpu().numpy(), wl), "exported leaf hashes differ"
        r = self.tree.root_device(stream=self.stream)
        torch.cuda.synchronize()
        assert r[0].cpu().numpy().tobytes() == want_root
        if against_root_call:
            full = self.stl.shamap_root_device(k.contiguous(), l.contiguous())
            torch.cuda.synchronize()
            assert full[0].cpu().numpy().tobytes() == want_root, "the full rebuild over the export disagrees"

    def step(self, keys, leaves=None, ops=None, against_root_call=False):
        want = self.m.apply(keys, leaves, ops)
        got = apply_guarded(self.torch, self.tree, keys, leaves, ops, self.stream)
        assert got[1] == want[1], (got[1], want[1])
        assert got[0] == want[0]
        self.check_content(want[0], against_root_call)
        return got

    def close(self):
        self.tree.close()


def _leaves(keys, seed):
    return np.random.default_rng(seed).integers(0, 256, np.asarray(keys).shape, dtype=np.uint8)


def _k(*rows):
    return np.ascontiguousarray(np.stack([np.frombuffer(bytes(r), np.uint8) for r in rows]))


# ---- 1. tiny trees ----
def test_tiny_trees(stl, torch_cuda):
    torch = torch_cuda
    rig = Rig(torch, stl, 16)
    info = rig.tree.info()
    assert (info["items"], info["root"], info["capacity"], info["bucket_depth"]) == (0, SM.ZERO, 16, 4)
    assert info["bytes"] >= 16 * 193
    rig.check_content(SM.ZERO)
    # n == 0 on the empty tree: the current root, the items and seven zeros
    assert apply_guarded(torch, rig.tree, np.zeros((0, 32), np.uint8)) == (SM.ZERO, [0] * 8)
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    b = a.copy()
    b[2:] = rng.integers(0, 256, 30, dtype=np.uint8)  # the same bucket, parting at nibble 4 or later
    b[2] = a[2] ^ 0x10
    la, lb = _leaves(a, 2), _leaves(b, 3)
    root, c = rig.step(_k(a), _k(la))
    assert c == [1, 1, 0, 0, 0, 0, 1, 1]
    assert root == SM.inner_hash([la.tobytes() if i == a[0] >> 4 else SM.ZERO for i in range(16)])
    two, c = rig.step(_k(b), _k(lb))
    assert c == [2, 1, 0, 0, 0, 0, 1, 2] and two != root
    assert apply_guarded(torch, rig.tree, np.zeros((0, 32), np.uint8)) == (two, [2, 0, 0, 0, 0, 0, 0, 0])
    # 2 -> 1 in the bucket: the leaf hash again, not an inner node; the chain collapses
    back, c = rig.step(_k(b), None, np.array([1], np.uint8))
    assert c == [1, 0, 0, 1, 0, 0, 1, 1] and back == root
    none, c = rig.step(_k(a), None, np.array([7], np.uint8))
    assert c == [0, 0, 0, 1, 0, 0, 1, 0] and none == SM.ZERO
    assert rig.tree.info()["items"] == 0
    rig.close()


# ---- 2. the golden sequences ----
def test_golden_sequences(stl, torch_cuda):
    with open(TM.GOLDEN) as f:
        doc = json.load(f)
    assert [s["name"] for s in doc["sequences"]] == TM.SEQUENCES
    for s in doc["sequences"]:
        rig = Rig(torch_cuda, stl, 2000)
        for b, want in zip(TM.sequence(s["name"]), s["steps"]):
            root, counts = rig.step(*b)
            assert (root.hex(), counts) == (want["root"], want["counts"]), s["name"]
        rig.close()


# ---- 3. a mixed sequence ----
def test_mixed_sequence(stl, torch_cuda):
    rng = np.random.default_rng(30)
    rig = Rig(torch_cuda, stl, 12000)
    keys = SM.case_keys("random5000", 31)
    rig.step(keys, _leaves(keys, 32))
    seen = [0] * 8
    for rows in (1, 37, 256, 700, 1500, 1024):
        _, c = rig.step(*TM._mixed_batch(rng, rig.m.items, rows))
        seen = [a + b for a, b in zip(seen, c)]
    assert all(seen[i] > 0 for i in range(1, 8)), seen  # every kind of change occurred
    rig.close()


# ---- 4. the bucket boundary ----
def _partner(key, shared, rng):
    """A key that shares exactly `shared` nibbles with key."""
    hx = key.tobytes().hex()
    other = "%x" % (int(hx[shared], 16) ^ (1 + int(rng.integers(0, 15))))
    tail = rng.integers(0, 256, 32, dtype=np.uint8).tobytes().hex()[shared + 1:]
    return np.frombuffer(bytes.fromhex(hx[:shared] + other + tail), np.uint8).copy()


def test_bucket_boundary(stl, torch_cuda):
    rng = np.random.default_rng(40)
    rig = Rig(torch_cuda, stl, 64)
    dele = np.array([1], np.uint8)
    for shared in (3, 4, 63, 0, 5, 62):  # 3: the node is the top kernel's; 4: the level path's
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        b = _partner(a, shared, rng)
        assert SM.common_prefix(a.tobytes(), b.tobytes()) == shared
        before = rig.m.root()
        rig.step(_k(a), _k(_leaves(a, shared)))
        rig.step(_k(b))
        rig.step(_k(a), None, dele)
        rig.step(_k(b), None, dele)
        assert rig.m.root() == before
    # the first and the last bucket, and the least and the greatest key
    zero, ones = np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8)
    lo = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    lo[:, :2] = 0
    hi = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    hi[:, :2] = 0xFF
    rig.step(_k(zero))
    rig.step(_k(ones), _k(_leaves(ones, 41)))
    rig.step(np.concatenate([lo, hi]), _leaves(np.concatenate([lo, hi]), 42))
    rig.step(_k(zero, ones, lo[0], hi[2]), None, np.array([1, 1, 0, 1], np.uint8))
    rig.step(np.concatenate([lo, hi]), None, np.ones(6, np.uint8))
    assert rig.m.root() == SM.ZERO
    rig.close()


# ---- 5. one bucket holding everything ----
@pytest.mark.parametrize("shape", ["dense", "cluster3000_5_62"])
def test_one_bucket_holds_everything(stl, torch_cuda, shape):
    keys = np.unique(SM.case_keys(shape, 50), axis=0)
    keys = keys[np.random.default_rng(51).permutation(keys.shape[0])]
    m = keys.shape[0]
    part = 3 * m // 4
    rig = Rig(torch_cuda, stl, m + 8)
    _, c = rig.step(keys[:part], _leaves(keys[:part], 52))
    assert c[0] == part and c[6] <= 5 and c[7] == part  # a handful of buckets, every leaf gathered
    # the rest inserted, an eighth deleted, an eighth replaced
    e = m // 8
    batch = np.concatenate([keys[part:], keys[:e], keys[e:2 * e]])
    ops = np.concatenate([np.zeros(m - part, np.uint8), np.ones(e, np.uint8), np.zeros(e, np.uint8)])
    _, c = rig.step(batch, _leaves(batch, 53), ops, against_root_call=True)
    assert c[:5] == [m - e, m - part, e, e, 0]
    rig.close()


# ---- 6. block and word edges ----
def _outside(rig, rows, above):
    """rows distinct keys wholly below the least resident key, or above the greatest."""
    ks = sorted(rig.m.items)
    lo, hi = int.from_bytes(ks[0], "big"), int.from_bytes(ks[-1], "big")
    if above:
        vals = [hi + (2 ** 256 - 1 - hi) * j // (rows + 1) for j in range(1, rows + 1)]
    else:
        vals = [lo * j // (rows + 1) for j in range(1, rows + 1)]
    assert len(set(vals)) == rows and all((v > hi) if above else (v < lo) for v in vals)
    return _k(*[v.to_bytes(32, "big") for v in vals])


@pytest.mark.parametrize("resident", [255, 256, 257, 65535, 65537, 131073])
def test_block_and_word_edges(stl, torch_cuda, resident):
    rng = np.random.default_rng(resident)
    small = resident < 1000
    rig = Rig(torch_cuda, stl, resident + 1 + 257 + 4097 + 600)
    keys = SM.case_keys(f"random{resident}", 60 + resident)
    rig.step(keys, _leaves(keys, 61), against_root_call=True)
    for rows in (1, 257, 4097):
        rig.step(*TM._mixed_batch(rng, rig.m.items, rows), against_root_call=True)
    below = _outside(rig, 257, above=False)
    rig.step(below, _leaves(below, 62), against_root_call=True)
    above = _outside(rig, 257 if small else 1, above=True)
    rig.step(above, None, np.zeros(above.shape[0], np.uint8), against_root_call=True)
    every, _ = rig.m.content()
    _, c = rig.step(every, _leaves(every, 63), against_root_call=True)  # replaces every item
    assert c[:5] == [every.shape[0], 0, every.shape[0], 0, 0]
    _, c = rig.step(every, None, np.ones(every.shape[0], np.uint8), against_root_call=True)  # deletes every item
    assert c[:5] == [0, 0, 0, every.shape[0], 0]
    rig.close()


# ---- 7. load ----
def test_load_equals_the_root_call(stl, torch_cuda):
    torch = torch_cuda
    keys = SM.case_keys("random131073", 70)
    lh = _leaves(keys, 71)
    rig = Rig(torch, stl, 131073)
    root, c = rig.step(keys, lh)
    assert c[:6] == [131073, 131073, 0, 0, 0, 0] and c[7] == 131073
    full, fc = stl.shamap_root_device(_dev(torch, keys), _dev(torch, lh), counts=True)
    torch.cuda.synchronize()
    assert full[0].cpu().numpy().tobytes() == root and int(fc[0]) == 131073
    rig.close()


# ---- 8. capacity ----
def test_capacity(stl, torch_cuda):
    from stellard_amd import _native as N
    torch = torch_cuda
    rig = Rig(torch, stl, 1000)
    keys = SM.case_keys("random2100", 80)
    root, _ = rig.step(keys[:600], _leaves(keys[:600], 81))

    def refused(rows, ops=None, rc=N.STL_ENOMEM):
        with pytest.raises(N.StlError) as e:
            apply_guarded(torch, rig.tree, rows, None, ops)
        assert e.value.rc == rc
        torch.cuda.synchronize()
        rig.check_content(rig.m.root())

    refused(keys[600:1001])  # 401 new keys: one too many
    assert rig.m.root() == root
    refused(keys[:1001], rc=N.STL_EINVAL)  # more rows than the capacity
    # the bound (600 + 600) runs out, the exact count does not: replaces need no room
    for seed in (82, 83):
        _, c = rig.step(keys[:600], _leaves(keys[:600], seed))
        assert c[:5] == [600, 0, 600, 0, 0]
    _, c = rig.step(keys[600:1000])  # exactly full, within the bound: no wait
    assert c[:2] == [1000, 400]
    refused(keys[1000:1001])
    # a full tree still takes deletes and what they make room for
    batch = np.concatenate([keys[:10], keys[1000:1010]])
    _, c = rig.step(batch, None, np.concatenate([np.ones(10, np.uint8), np.zeros(10, np.uint8)]))
    assert c[:5] == [1000, 10, 0, 10, 0]
    refused(keys[1010:1011])
    _, c = rig.step(keys[:1000], None, np.ones(1000, np.uint8))  # the first ten are gone already
    assert c[:5] == [10, 0, 0, 990, 10]
    assert rig.tree.info()["items"] == 10
    rig.close()


# ---- 9. injected errors ----
def test_fault_injection(stl, torch_cuda):
    """Every HIP call of one device apply and of one host apply failed in turn
    (at the API boundary: no device fault): the call returns < 0 and leaves its
    outputs, the root and the content alone, and the same batch applied
    afterwards gives the model's result."""
    from stellard_amd import _native as N
    torch = torch_cuda
    rng = np.random.default_rng(90)
    rig = Rig(torch, stl, 4000, stream=torch.cuda.Stream())  # a fresh context: the first call also allocates
    keys = SM.case_keys("random300", 91)
    rig.step(keys, _leaves(keys, 92))
    for form in ("device", "host"):
        failed, kk = 0, 0
        try:
            while True:
                assert kk < 250, "the countdown never ran out"
                batch = TM._mixed_batch(rng, rig.m.items, 40)
                before = rig.m.root()
                dev = [_dev(torch, a) for a in batch]
                root = torch.full((1, 32), GUARD, dtype=torch.uint8, device="cuda")
                cnt = torch.full((8,), GUARD_WORD, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                stl.debug_fault_after(kk)
                kk += 1
                try:
                    if form == "device":
                        rig.tree.apply_device(*dev, out_root=root, counts=cnt, stream=rig.stream)
                        torch.cuda.synchronize()
                        got = (root[0].cpu().numpy().tobytes(), [int(x) for x in cnt.cpu().numpy()])
                    else:
                        got = rig.tree.apply(*batch, counts=True)
                except N.StlError as e:
                    assert e.rc < 0
                    failed += 1
                    stl.debug_fault_after(-1)
                    torch.cuda.synchronize()
                    assert (root == GUARD).all() and (cnt == GUARD_WORD).all(), kk
                    rig.check_content(before)  # root and export unchanged
                    rig.step(*batch)  # the same batch, clean
                    continue
                stl.debug_fault_after(-1)
                assert got == rig.m.apply(*batch)
                rig.check_content(got[0])
                break  # no call left to fail
        finally:
            stl.debug_fault_after(-1)
        torch.cuda.synchronize()
        # the memsets, 4 word kernels and sorts, head, scan, compact, locate, scan, 2 merges, bounds,
        # sizes, scan, gather, neighbours, 60 levels, bucket values, 4 top launches, finish
        assert failed == kk - 1 and failed >= 88, (form, failed)
    rig.close()


# ---- 10. streams and handles ----
def test_streams_and_handles(stl, torch_cuda):
    from stellard_amd import _native as N
    torch = torch_cuda
    rng = np.random.default_rng(100)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = Rig(torch, stl, 6000, stream=s1), Rig(torch, stl, 3000, stream=s2)
    ka, kb = SM.case_keys("random4097", 101), SM.case_keys("cluster2000_9_20", 102)
    a.step(ka, _leaves(ka, 103))
    b.step(kb)
    for rows in (64, 300, 5):  # interleaved, each on its own stream
        a.step(*TM._mixed_batch(rng, a.m.items, rows))
        b.step(*TM._mixed_batch(rng, b.m.items, rows + 1))
    # several applies enqueued back to back on one stream, no wait between them
    batches = [TM._mixed_batch(rng, a.m.items, 50) for _ in range(3)]
    dev = [[_dev(torch, x) for x in bt] for bt in batches]
    torch.cuda.synchronize()
    outs = [a.tree.apply_device(*d, counts=True, stream=s1) for d in dev]
    torch.cuda.synchronize()
    for bt, (r, c) in zip(batches, outs):
        assert (r[0].cpu().numpy().tobytes(), [int(x) for x in c.cpu()]) == a.m.apply(*bt)
    a.check_content(a.m.root())
    # the host form equals the device form
    host = stl.ShamapTree(6000)
    hm = TM.Model()
    assert host.apply(np.zeros((0, 32), np.uint8), counts=True) == (SM.ZERO, [0] * 8)
    for bt in [(ka, _leaves(ka, 103), None)] + [TM._mixed_batch(rng, a.m.items, 200)]:
        assert host.apply(*bt, counts=True) == hm.apply(*bt)
    assert host.apply(ka[:3], ops=np.array([True, False, True])) == hm.apply(ka[:3], None, [1, 0, 1])[0]
    assert host.info()["items"] == len(hm.items) and host.info()["root"] == hm.root()
    # a destroyed handle
    h = ctypes.c_void_p(host.handle.value)
    host.close()
    root = torch.zeros((1, 32), dtype=torch.uint8, device="cuda")
    lib = N.load()
    assert lib.stl_shamap_tree_root_device(h, ctypes.c_void_p(root.data_ptr()), None) == N.STL_EINVAL
    assert lib.stl_shamap_tree_apply_device(h, ctypes.c_void_p(root.data_ptr()), None, None, 1,
                                            ctypes.c_void_p(root.data_ptr()), None, None) == N.STL_EINVAL
    lib.stl_shamap_tree_destroy(h)  # ignored
    a.close()
    b.close()
    # stl_shutdown frees every tree: the handle is dead afterwards, a new tree starts empty
    left = stl.ShamapTree(64)
    want = TM.Model().apply(ka[:5])
    assert left.apply(ka[:5], counts=True) == want
    h = ctypes.c_void_p(left.handle.value)
    stl.shutdown()
    stl.init()
    assert lib.stl_shamap_tree_root_device(h, ctypes.c_void_p(root.data_ptr()), None) == N.STL_EINVAL
    left.close()  # ignored
    with stl.ShamapTree(64) as again:
        assert again.info()["items"] == 0 and again.apply(ka[:5], counts=True) == want
