"""GPU tests of the resident SHAMap's fork and revert (stl_shamap_tree_fork*,
stl_shamap_tree_revert): after a fork the destination's root, counts and
exported content equal the model of tests/shamap_fork_py.py (the tree model
copied, then applied) and the source is byte-equal to what it was; a revert
gives back what the tree held before its last successful apply or fork.

Run on an MI355X:  python -u -m pytest tests/test_gpu_shamap_fork.py -m gpu -x -v
"""
import numpy as np
import pytest

from tests import shamap_fork_py as FM
from tests import shamap_nodes_py as NM
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
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.shape[0] == 0:
        return torch.zeros(a.shape, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a).cuda()


def _leaves(keys, seed):
    return np.random.default_rng(seed).integers(0, 256, np.asarray(keys).shape, dtype=np.uint8)


class Tree:
    """A tree on the device with its capacity; the model travels beside it."""

    def __init__(self, torch, stl, capacity, keys=None, leaves=None):
        self.torch, self.stl, self.cap = torch, stl, capacity
        self.tree = stl.ShamapTree(capacity)
        self.m = TM.Model()
        if keys is not None and len(keys):
            self.apply(keys, leaves)

    def apply(self, keys, leaves=None, ops=None, stream=None):
        """One device apply, checked against the model."""
        torch = self.torch
        want = self.m.apply(keys, leaves, ops)
        r, c = self.tree.apply_device(_dev(torch, keys), _dev(torch, leaves), _dev(torch, ops), counts=True,
                                      stream=stream)
        torch.cuda.synchronize()
        assert (r[0].cpu().numpy().tobytes(), [int(x) for x in c.cpu()]) == want
        return want

    def content(self, stream=None):
        """Export on guarded buffers and the root -> (keys, leaf hashes, root) as bytes.  Reads no count on the host."""
        torch, rows = self.torch, self.cap
        k = torch.full((rows + 2, 32), GUARD, dtype=torch.uint8, device="cuda")
        l = torch.full((rows + 2, 32), GUARD, dtype=torch.uint8, device="cuda")
        items = torch.full((3,), GUARD_WORD, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.tree.export_device(k[1:rows + 1], l[1:rows + 1], items[1:2], stream=stream)
        r = self.tree.root_device(stream=stream)
        torch.cuda.synchronize()
        m = int(items[1])
        assert int(items[0]) == GUARD_WORD and int(items[2]) == GUARD_WORD and 0 <= m <= rows
        for t in (k, l):
            assert (t[0] == GUARD).all() and (t[m + 1:] == GUARD).all(), "rows beside the content overwritten"
        self.last = (k[1:m + 1], l[1:m + 1])
        return k[1:m + 1].cpu().numpy().tobytes(), l[1:m + 1].cpu().numpy().tobytes(), r[0].cpu().numpy().tobytes()

    def check(self, model=None, against_root_call=False):
        """The content equals the model's sorted dict and root."""
        model = self.m if model is None else model
        wk, wl = model.content()
        got = self.content()
        assert got == (wk.tobytes(), wl.tobytes(), model.root())
        if against_root_call and len(model.items):
            full = self.stl.shamap_root_device(self.last[0].contiguous(), self.last[1].contiguous())
            self.torch.cuda.synchronize()
            assert full[0].cpu().numpy().tobytes() == model.root(), "the full rebuild over the export disagrees"
        return got

    def fork(self, dst, keys=None, leaves=None, ops=None, stream=None):
        """One device fork into dst on guarded outputs, against the model; dst's model follows."""
        torch = self.torch
        want, root, counts = FM.fork(self.m, keys, leaves, ops)
        r = torch.full((3, 32), GUARD, dtype=torch.uint8, device="cuda")
        c = torch.full((24,), GUARD_WORD, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.tree.fork_device(dst.tree, _dev(torch, keys), _dev(torch, leaves), _dev(torch, ops), out_root=r[1:2],
                              counts=c[8:16], stream=stream)
        torch.cuda.synchronize()
        assert (r[0] == GUARD).all() and (r[2] == GUARD).all(), "guard bytes beside the root overwritten"
        assert (c[:8] == GUARD_WORD).all() and (c[16:] == GUARD_WORD).all(), "guard words beside the counts overwritten"
        assert [int(x) for x in c[8:16].cpu()] == counts
        assert r[1].cpu().numpy().tobytes() == root
        dst.m = want
        return root, counts

    def differences(self, other):
        d = self.tree.compare(other.tree, 0)
        return d.counts[:4]

    def close(self):
        self.tree.close()


def _want_difference(a, b):
    only_a, only_b, changed = FM.difference(a.items, b.items)
    return [only_a + only_b + changed, only_a, only_b, changed]


def _refused(fn, rc):
    from stellard_amd import _native as N
    with pytest.raises(N.StlError) as e:
        fn()
    assert e.value.rc == rc


# ---- 1. the snapshot ----
@pytest.mark.parametrize("items", [0, 1, 2, 255, 256, 257, 65537, 131073])
def test_snapshot(stl, torch_cuda, items):
    torch = torch_cuda
    keys = SM.case_keys(f"random{items}", 10 + items) if items else np.zeros((0, 32), np.uint8)
    src = Tree(torch, stl, items + 3, keys, _leaves(keys, 11))
    old = SM.case_keys("random40", 12)
    dst = Tree(torch, stl, items + 70, old)  # what it held is replaced
    before = src.check()
    root, counts = src.fork(dst)
    assert counts == [items] + [0] * 7 and root == src.m.root()
    assert dst.check(against_root_call=True) == before == src.content()
    si, di = src.tree.info(), dst.tree.info()
    assert (di["items"], di["root"]) == (si["items"], si["root"]) == (items, root)
    assert (di["capacity"], si["capacity"]) == (items + 70, items + 3)
    assert src.differences(dst) == [0, 0, 0, 0]
    # a snapshot is a tree of its own: changing it leaves the source alone
    dst.apply(old[:5], _leaves(old[:5], 13))
    dst.check()
    assert src.content() == before
    src.close()
    dst.close()


# ---- 2. a fork with a batch ----
def test_fork_with_a_batch(stl, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(20)
    keys = SM.case_keys("random5000", 21)
    src = Tree(torch, stl, 6000, keys, _leaves(keys, 22))
    dst = Tree(torch, stl, 7000)
    probes = np.concatenate([keys[rng.integers(0, 5000, 700)], rng.integers(0, 256, (300, 32), dtype=np.uint8)])
    looked = src.tree.lookup(probes, leaf_hashes=True, positions=True)
    before = src.check()
    seen = [0] * 8
    for rows in (1, 37, 700, 1500):
        _, c = src.fork(dst, *TM._mixed_batch(rng, src.m.items, rows))
        seen = [a + b for a, b in zip(seen, c)]
        dst.check(against_root_call=True)
        assert src.differences(dst) == _want_difference(src.m, dst.m)
        assert src.content() == before
        again = src.tree.lookup(probes, leaf_hashes=True, positions=True)
        assert all(np.array_equal(a, b) for a, b in zip(looked, again))
    assert all(seen[i] > 0 for i in range(1, 8)), seen  # inserts, replaces, deletes, absent deletes, superseded rows
    src.check()
    src.close()
    dst.close()


# ---- 3. shapes ----
@pytest.mark.parametrize("name", ["bucket_boundary", "one_bucket", "collapse_2_to_1", "empties_the_tree", "mixed_batch"])
def test_shapes(stl, torch_cuda, name):
    model, batch = FM.case(name)
    sk, sl = model.content()
    src = Tree(torch_cuda, stl, len(model.items) + 1, sk, sl)
    dst = Tree(torch_cuda, stl, len(model.items) + len(batch[0]), SM.case_keys("random3", 30))
    before = src.check()
    src.fork(dst, *batch)
    dst.check(against_root_call=True)
    assert src.content() == before
    assert src.differences(dst) == _want_difference(src.m, dst.m)
    src.close()
    dst.close()


def test_one_bucket_holds_everything(stl, torch_cuda):
    keys = np.unique(SM.case_keys("dense", 31), axis=0)
    keys = keys[np.random.default_rng(32).permutation(keys.shape[0])]
    m = keys.shape[0]
    part, e = 3 * m // 4, m // 8
    src = Tree(torch_cuda, stl, m, keys[:part], _leaves(keys[:part], 33))
    dst = Tree(torch_cuda, stl, m + 8)
    batch = np.concatenate([keys[part:], keys[:e], keys[e:2 * e]])
    ops = np.concatenate([np.zeros(m - part, np.uint8), np.ones(e, np.uint8), np.zeros(e, np.uint8)])
    before = src.content()
    _, c = src.fork(dst, batch, _leaves(batch, 34), ops)
    assert c[:5] == [m - e, m - part, e, e, 0] and c[6] <= 5
    dst.check(against_root_call=True)
    assert src.content() == before
    src.close()
    dst.close()


# ---- 4. capacities ----
def test_capacities(stl, torch_cuda):
    from stellard_amd import _native as N
    torch = torch_cuda
    keys = SM.case_keys("random2100", 40)
    src = Tree(torch, stl, 1000, keys[:600], _leaves(keys[:600], 41))
    # the destination smaller than the source's capacity, large enough for the bound: no wait
    small = Tree(torch, stl, 700)
    src.fork(small, keys[600:700])
    small.check(against_root_call=True)
    # the source's bound loose after deletes (600 + 300 rows): the wait path runs, and the exact count fits
    src.apply(keys[:300], None, np.ones(300, np.uint8))
    before = src.content()
    tight = Tree(torch, stl, 400, keys[2000:2010])
    src.fork(tight, keys[600:650])                      # 300 + 50 into 400
    tight.check(against_root_call=True)
    src.fork(tight)                                     # the snapshot's wait: 300 into 400
    tight.check()
    src.fork(tight, keys[600:700])                      # a result of exactly the capacity
    assert len(tight.m.items) == 400
    tight.check(against_root_call=True)
    held, held_model = tight.content(), tight.m
    # one over: STL_ENOMEM, both trees unchanged -- and no revert into the refused call's work
    dk = _dev(torch, keys[600:701])
    _refused(lambda: src.tree.fork_device(tight.tree, dk), N.STL_ENOMEM)
    torch.cuda.synchronize()
    assert tight.content() == held and src.content() == before
    _refused(tight.tree.revert, N.STL_EINVAL)
    exact = Tree(torch, stl, 299)
    _refused(lambda: src.tree.fork_device(exact.tree), N.STL_ENOMEM)  # a snapshot that does not fit
    _refused(lambda: src.tree.fork(exact.tree), N.STL_ENOMEM)
    torch.cuda.synchronize()
    assert exact.content() == (b"", b"", SM.ZERO) and src.content() == before
    # more rows than the destination holds: an argument error, nothing begun
    _refused(lambda: src.tree.fork_device(tight.tree, _dev(torch, keys[:401])), N.STL_EINVAL)
    tight.m = held_model
    src.fork(tight, keys[300:400], None, np.ones(100, np.uint8))  # a full destination is simply replaced
    tight.check()
    for t in (src, small, tight, exact):
        t.close()


# ---- 5. generations ----
@pytest.mark.parametrize("handles", [2, 3])
def test_chain_of_forks(stl, torch_cuda, handles):
    """a -> b -> a ... over two handles, a -> b -> c -> a ... over three: six forks, each against the model."""
    rng = np.random.default_rng(50 + handles)
    keys = SM.case_keys("random3000", 51)
    trees = [Tree(torch_cuda, stl, 4000 + 100 * i) for i in range(handles)]
    trees[0].apply(keys, _leaves(keys, 52))
    for step in range(6):
        src, dst = trees[step % handles], trees[(step + 1) % handles]
        before = src.content()
        rows = (0, 300, 1, 257, 64, 700)[step] if handles == 2 else (64, 0, 300, 1, 0, 500)[step]
        batch = TM._mixed_batch(rng, src.m.items, rows) if rows else (None, None, None)
        src.fork(dst, *batch)
        dst.check(against_root_call=True)
        assert src.content() == before
    for t in trees:
        t.close()


def test_two_forks_of_one_source_on_two_streams(stl, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(55)
    keys = SM.case_keys("random65537", 56)
    src = Tree(torch, stl, 70000, keys, _leaves(keys, 57))
    a, b = Tree(torch, stl, 70000), Tree(torch, stl, 66000)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ba, bb = TM._mixed_batch(rng, src.m.items, 400), TM._mixed_batch(rng, src.m.items, 257)
    da, db = [_dev(torch, x) for x in ba], [_dev(torch, x) for x in bb]
    before = src.content()
    torch.cuda.synchronize()
    ra = src.tree.fork_device(a.tree, *da, counts=True, stream=s1)  # enqueued back to back, no wait between them
    rb = src.tree.fork_device(b.tree, *db, counts=True, stream=s2)
    torch.cuda.synchronize()
    for t, batch, (r, c) in ((a, ba, ra), (b, bb, rb)):
        t.m, root, counts = FM.fork(src.m, *batch)
        assert (r[0].cpu().numpy().tobytes(), [int(x) for x in c.cpu()]) == (root, counts)
        t.check()
    assert src.content() == before
    for t in (src, a, b):
        t.close()


# ---- 6. the revert ----
def test_the_source_keeps_its_revert_state(stl, torch_cuda):
    keys = SM.case_keys("random600", 60)
    src = Tree(torch_cuda, stl, 800, keys[:400], _leaves(keys[:400], 61))
    pre = src.content()
    earlier = TM.Model()
    earlier.items = dict(src.m.items)
    src.apply(keys[300:500], None, (np.arange(200) % 2).astype(np.uint8))
    dst = Tree(torch_cuda, stl, 800)
    src.fork(dst, keys[500:])
    src.tree.revert()
    assert src.content() == pre
    src.m = earlier
    src.check(against_root_call=True)
    dst.check()
    src.close()
    dst.close()


def test_revert(stl, torch_cuda):
    from stellard_amd import _native as N
    torch = torch_cuda
    keys = SM.case_keys("random1200", 62)
    probes = keys[::3].copy()
    t = Tree(torch, stl, 1500)
    _refused(t.tree.revert, N.STL_EINVAL)  # a fresh tree
    t.apply(keys[:700], _leaves(keys[:700], 63))
    first, first_model = t.content(), dict(t.m.items)
    looked = t.tree.lookup(probes, leaf_hashes=True, positions=True)
    # after an apply
    t.apply(keys[600:900], None, (np.arange(300) % 3 == 0).astype(np.uint8))
    assert t.tree.info()["items"] == len(t.m.items) != 700  # get_info between the apply and the revert
    t.tree.revert()
    assert t.content() == first and t.tree.info()["items"] == 700
    assert all(np.array_equal(a, b) for a, b in zip(looked, t.tree.lookup(probes, leaf_hashes=True, positions=True)))
    _refused(t.tree.revert, N.STL_EINVAL)  # one step only
    t.m.items = dict(first_model)
    # an apply of no rows changes nothing, the revert state included
    t.apply(keys[900:1000])
    t.tree.apply_device(torch.zeros((0, 32), dtype=torch.uint8, device="cuda"))
    t.tree.revert()
    t.m.items = dict(first_model)
    assert t.content() == first
    # after a fork into it
    src = Tree(torch, stl, 400, keys[1000:1200])
    src.fork(t, keys[:50])
    t.check()
    t.tree.revert()
    t.m.items = dict(first_model)
    assert t.content() == first
    _refused(t.tree.revert, N.STL_EINVAL)
    # revert, then an apply: the root call over the export agrees
    t.apply(keys[650:800], _leaves(keys[650:800], 64))
    t.check(against_root_call=True)
    t.tree.revert()
    t.m.items = dict(first_model)
    t.apply(keys[100:200], None, np.ones(100, np.uint8))
    t.check(against_root_call=True)
    # the host form
    src.tree.fork(t.tree)
    t.tree.revert()
    t.check()
    # a handle that is not live
    dead = stl.ShamapTree(16)
    h = dead.handle.value
    dead.close()
    assert N.load().stl_shamap_tree_revert(h) == N.STL_EINVAL
    src.close()
    t.close()


# ---- 7. the nodes forms ----
def _node_rows(nodes):
    rows = nodes.rows()
    return NM.rows_as_dict(rows, nodes.hash.cpu().numpy(), nodes.body.cpu().numpy(), nodes.ids.cpu().numpy(),
                           nodes.meta.cpu().numpy())


def test_fork_nodes(stl, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(70)
    keys = SM.case_keys("random3000", 71)
    src = Tree(torch, stl, 3500, keys, _leaves(keys, 72))
    dst = Tree(torch, stl, 4000, keys[:9])
    before = src.content()
    batch = TM._mixed_batch(rng, src.m.items, 300)
    want, root, counts = FM.fork(src.m, *batch)
    e = NM.emitted(want.items, batch[0])  # the source is the old tree: the dirty buckets and the prefixes above them
    dev = [_dev(torch, x) for x in batch]
    for max_nodes in (len(e) + 5, 0, len(e) - 1):  # all of them; overflow at 0 and at count - 1
        r, c, nodes = src.tree.fork_nodes_device(dst.tree, *dev, max_nodes=max_nodes)
        torch.cuda.synchronize()
        assert (r[0].cpu().numpy().tobytes(), [int(x) for x in c.cpu()]) == (root, counts)
        assert int(nodes.count.item()) == len(e)
        got = _node_rows(nodes) if max_nodes else {}
        assert len(got) == min(max_nodes, len(e)) and all(e[k] == v for k, v in got.items())
        dst.check(want)
        assert src.content() == before
    # the host form, and no rows: no node, a count of zero
    hroot, hcounts, hn = src.tree.fork_nodes(dst.tree, *batch, max_nodes=len(e))
    assert (hroot, hcounts, hn.count) == (root, counts, len(e))
    assert NM.rows_as_dict(hn.rows(), hn.hash, hn.body, hn.ids, hn.meta) == e
    dst.check(want)
    hroot, hcounts, hn = src.tree.fork_nodes(dst.tree, max_nodes=4)
    assert (hroot, hcounts, hn.count) == (src.m.root(), [3000] + [0] * 7, 0)
    r, c, nodes = src.tree.fork_nodes_device(dst.tree, max_nodes=4)
    torch.cuda.synchronize()
    assert int(nodes.count.item()) == 0 and [int(x) for x in c.cpu()] == [3000] + [0] * 7
    dst.check(src.m)
    assert src.content() == before
    src.close()
    dst.close()


# ---- 8. the host forms and parity with the apply ----
def test_host_form_and_parity_with_the_apply(stl, torch_cuda):
    """The existing apply on the same inputs gives the root and counts of a fork followed by reading dst."""
    rng = np.random.default_rng(80)
    keys = SM.case_keys("random4097", 81)
    lh = _leaves(keys, 82)
    src = Tree(torch_cuda, stl, 5000, keys, lh)
    twin = Tree(torch_cuda, stl, 5000, keys, lh)
    dst = Tree(torch_cuda, stl, 6000)
    for rows in (257, 1, 1000):
        batch = TM._mixed_batch(rng, src.m.items, rows)
        root, counts = src.fork(dst, *batch)
        assert src.tree.fork(dst.tree, *batch, counts=True) == (root, counts)  # the host form, the same again
        assert twin.apply(*batch) == (root, counts)
        assert dst.content() == twin.content()
        info = dst.tree.info()
        assert (info["items"], info["root"]) == (counts[0], root)
        assert twin.differences(dst) == [0, 0, 0, 0]
        src.fork(dst)  # ... and the two go on from the same tree
        twin.tree.revert()
        twin.m.items = dict(src.m.items)
        assert twin.content() == src.content()
    assert src.tree.fork(dst.tree, counts=True) == (src.m.root(), [4097] + [0] * 7)
    for t in (src, twin, dst):
        t.close()


# ---- 9. injected errors ----
@pytest.mark.parametrize("form", ["rows", "snapshot", "wait", "snapshot_wait", "host_rows", "host_snapshot"])
def test_fault_injection(stl, torch_cuda, form):
    """Every HIP call of one fork failed in turn (at the API boundary: no device
    fault): the call returns < 0 and leaves its outputs, the destination and the
    source alone, a revert of the destination is refused, and the same fork
    afterwards gives the model's result."""
    from stellard_amd import _native as N
    torch = torch_cuda
    rng = np.random.default_rng(90)
    keys = SM.case_keys("random700", 91)
    stream = torch.cuda.Stream()  # a fresh context: the first call also allocates
    src = Tree(torch, stl, 1000, keys[:600], _leaves(keys[:600], 92))
    waits = form in ("wait", "snapshot_wait")
    if waits:  # the source's bound loose: 600 + 300 against a destination of 500
        src.apply(keys[:300], None, np.ones(300, np.uint8))
    dst = Tree(torch, stl, 500 if waits else 1000, keys[600:610])
    before = src.content()
    failed, kk = 0, 0
    try:
        while True:
            assert kk < 250, "the countdown never ran out"
            batch = (None, None, None) if "snapshot" in form else TM._mixed_batch(rng, src.m.items, 40)
            held = dst.content()
            dev = [_dev(torch, a) for a in batch]
            root = torch.full((1, 32), GUARD, dtype=torch.uint8, device="cuda")
            cnt = torch.full((8,), GUARD_WORD, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            stl.debug_fault_after(kk)
            kk += 1
            try:
                if form.startswith("host"):
                    got = src.tree.fork(dst.tree, *batch, counts=True)
                else:
                    src.tree.fork_device(dst.tree, *dev, out_root=root, counts=cnt, stream=stream)
                    torch.cuda.synchronize()
                    got = (root[0].cpu().numpy().tobytes(), [int(x) for x in cnt.cpu().numpy()])
            except N.StlError as e:
                assert e.rc < 0
                failed += 1
                stl.debug_fault_after(-1)
                torch.cuda.synchronize()
                assert (root == GUARD).all() and (cnt == GUARD_WORD).all(), kk
                assert dst.content() == held and src.content() == before, kk
                _refused(dst.tree.revert, N.STL_EINVAL)  # the failed call's generation is what it would expose
                src.fork(dst, *batch, stream=stream)  # the same fork, clean
                dst.check()
                if "snapshot" in form:  # a snapshot gives the same tree every time: make the next one visible
                    dst.apply(keys[610 + kk % 50:611 + kk % 50])
                continue
            stl.debug_fault_after(-1)
            want, wroot, wcounts = FM.fork(src.m, *batch)
            assert got == (wroot, wcounts)
            dst.check(want)
            break  # no call left to fail
    finally:
        stl.debug_fault_after(-1)
    torch.cuda.synchronize()
    assert failed == kk - 1 and src.content() == before
    # a snapshot is two launches; a fork with rows is the apply's sequence: the memsets, the sorts, head, scan,
    # compact, locate, scan, 2 merges, bounds, sizes, scan, gather, neighbours, 60 levels, bucket values, 4 top
    # launches, finish; the waiting path adds two copies and the wait
    least = {"rows": 88, "wait": 91, "snapshot": 2, "snapshot_wait": 4, "host_rows": 88, "host_snapshot": 2}[form]
    assert failed >= least, (form, failed)
    src.close()
    dst.close()


def test_a_failed_apply_refuses_the_revert(stl, torch_cuda):
    """An injected error in an apply that follows a good apply: the content is
    the good apply's, and a revert -- which would expose the failed call's
    half-written generation -- is refused until the next good call."""
    from stellard_amd import _native as N
    torch = torch_cuda
    keys = SM.case_keys("random900", 95)
    t = Tree(torch, stl, 1000, keys[:300], _leaves(keys[:300], 96))
    t.apply(keys[300:600])
    good = t.content()
    dev = _dev(torch, keys[600:900])
    for after in (30, 70):  # in the sort passes; in the level launches, the merge already written
        stl.debug_fault_after(after)
        try:
            with pytest.raises(N.StlError) as e:
                t.tree.apply_device(dev)
            assert e.value.rc < 0
        finally:
            stl.debug_fault_after(-1)
        torch.cuda.synchronize()
        assert t.content() == good
        _refused(t.tree.revert, N.STL_EINVAL)
    t.check()
    t.apply(keys[600:900])  # the next good call: one step back is the good apply again
    t.tree.revert()
    assert t.content() == good
    t.close()
