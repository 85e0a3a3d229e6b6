"""GPU tests of a resident SHAMap's nodes by node ID and paths by key
(stl_shamap_tree_get_nodes*): on guarded outputs every request's rows are, in
order -- hash, body, ID and meta all compared -- the model of
tests/shamap_get_py.py, and so are status, first, rows, leaf key, leaf hash and
the eight counts; the tree is byte-equal to what it was.

Run on an MI355X:  python -u -m pytest tests/test_gpu_shamap_get.py -m gpu -x -v
"""
import ctypes
import json

import numpy as np
import pytest

from tests import shamap_get_py as GM
from tests import shamap_lookup_py as LM
from tests import shamap_nodes_py as NM

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
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.shape[0] == 0:
        return torch.zeros(a.shape, dtype=a.dtype == np.uint8 and torch.uint8 or torch.int32, device="cuda")
    return torch.from_numpy(a).cuda()


def _tree(stl, torch, items, capacity=None):
    """A resident tree holding {key: leaf hash}, built by the existing apply."""
    t = stl.ShamapTree(capacity if capacity is not None else max(len(items), 1))
    if items:
        k, l = LM.arrays(items)
        t.apply_device(_dev(torch, k), _dev(torch, l))
    return t


class Guarded:
    """Every output of one call with a guard row either side: the node arrays of
    max_nodes rows, the per-request arrays of n entries, guard words round the
    count and the counts."""

    def __init__(self, stl, torch, n, max_nodes, ids=True, meta=True, leaves=True, counts=True):
        self.torch, self.n, self.max_nodes = torch, n, max_nodes
        rows, nn = max(max_nodes, 1), max(n, 1)
        u8 = lambda r, w: torch.full((r + 2, w), GUARD, dtype=torch.uint8, device="cuda")  # noqa: E731
        i32 = lambda r: torch.full((r + 2,), GUARD_WORD, dtype=torch.int32, device="cuda")  # noqa: E731
        self.hash, self.body = u8(rows, 32), u8(rows, 512)
        self.ids = u8(rows, 32) if ids else None
        self.meta = i32(rows) if meta else None
        self.count = i32(1)
        self.counts = torch.full((24,), GUARD_WORD, dtype=torch.int32, device="cuda") if counts else None
        self.status = torch.full((nn + 32,), GUARD, dtype=torch.uint8, device="cuda")  # 16 guard bytes either side
        self.first, self.rows = i32(nn), i32(nn)
        self.leaf_key = u8(nn, 32) if leaves else None
        self.leaf_hash = u8(nn, 32) if leaves else None
        inner = lambda t: False if t is None else t[1:rows + 1]  # noqa: E731
        self.nodes = stl.DeviceNodes(max_nodes, ids=inner(self.ids), meta=inner(self.meta), hash=inner(self.hash),
                                     body=inner(self.body), count=self.count[1:2])

    def call(self, tree, ids, depths, modes, stream=None):
        """The C entry point on the interior of the guarded arrays -> its return code."""
        from stellard_amd import _native as N
        p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else None  # noqa: E731
        out = self.nodes.struct()
        s = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
        return N.load().stl_shamap_tree_get_nodes_device(
            tree.handle, p(ids), p(depths), p(modes), self.n, p(self.status, 16), p(self.first, 4), p(self.rows, 4),
            p(self.leaf_key, 32), p(self.leaf_hash, 32), ctypes.byref(out), p(self.counts, 32), s)

    def untouched(self):
        """What a failed call must leave of the count words."""
        c = self.counts is None or bool((self.counts == GUARD_WORD).all())
        return c and bool((self.count == GUARD_WORD).all())

    def read(self):
        """Waits; checks every guard -> the arguments of shamap_get_py.check_outputs."""
        torch, room, n = self.torch, self.max_nodes, self.n
        torch.cuda.synchronize()
        count = int(self.count[1]) & 0xFFFFFFFF
        assert int(self.count[0]) == GUARD_WORD and int(self.count[2]) == GUARD_WORD
        stored = min(count, room)
        for t in (self.hash, self.body, self.ids):
            if t is not None:
                assert (t[0] == GUARD).all() and (t[stored + 1:] == GUARD).all(), "a store past the rows written"
        if self.meta is not None:
            assert int(self.meta[0]) == GUARD_WORD and (self.meta[stored + 1:] == GUARD_WORD).all()
        counts = None
        if self.counts is not None:
            assert (self.counts[:8] == GUARD_WORD).all() and (self.counts[16:] == GUARD_WORD).all()
            counts = [int(x) for x in self.counts[8:16].cpu()]
        assert (self.status[:16] == GUARD).all() and (self.status[16 + n:] == GUARD).all()
        for t in (self.first, self.rows):
            assert int(t[0]) == GUARD_WORD and (t[n + 1:] == GUARD_WORD).all()
        for t in (self.leaf_key, self.leaf_hash):
            if t is not None:
                assert (t[0] == GUARD).all() and (t[n + 1:] == GUARD).all()
        np_ = lambda t, a, b: None if t is None else t[a:b].cpu().numpy()  # noqa: E731
        return (np_(self.status, 16, 16 + n), np_(self.first, 1, n + 1).astype(np.int64) & 0xFFFFFFFF,
                np_(self.rows, 1, n + 1).astype(np.int64) & 0xFFFFFFFF, np_(self.leaf_key, 1, n + 1),
                np_(self.leaf_hash, 1, n + 1), np_(self.hash, 1, stored + 1), np_(self.body, 1, stored + 1),
                np_(self.ids, 1, stored + 1), np_(self.meta, 1, stored + 1), count, counts)


def _get(stl, torch, tree, requests, modes=True, max_nodes=None, stream=None, **kw):
    """One device call on guarded outputs, enqueued; read() waits."""
    rid, rdepth, rmode = GM.request_arrays(requests)
    if max_nodes is None:
        max_nodes = GM.MAX_ROWS * len(requests)
    g = Guarded(stl, torch, len(requests), max_nodes, **kw)
    g.inputs = (_dev(torch, rid), _dev(torch, rdepth), _dev(torch, rmode) if modes else None)
    torch.cuda.synchronize()
    rc = g.call(tree, *g.inputs, stream=stream)
    assert rc == 0, rc
    return g


def _check(ans, g):
    GM.check_outputs(ans, *g.read())


def _content(torch, tree, rows):
    k = torch.full((rows + 1, 32), GUARD, dtype=torch.uint8, device="cuda")
    l = torch.full((rows + 1, 32), GUARD, dtype=torch.uint8, device="cuda")
    items = tree.export_device(k[:rows], l[:rows])
    r = tree.root_device()
    torch.cuda.synchronize()
    assert (k[rows] == GUARD).all() and (l[rows] == GUARD).all()
    m = int(items[0])
    return k[:m].cpu().numpy().tobytes(), l[:m].cpu().numpy().tobytes(), r[0].cpu().numpy().tobytes()


def _random_items(n, seed):
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 256, (n, 32), dtype=np.uint8), axis=0)
    assert len(keys) == n
    leaves = rng.integers(0, 256, keys.shape, dtype=np.uint8)
    return {k.tobytes(): v.tobytes() for k, v in zip(keys, leaves)}


# ---- 1. the named cases ----
@pytest.mark.parametrize("name", GM.CASES)
def test_named_cases(stl, torch_cuda, name):
    torch = torch_cuda
    items, requests, modes = GM.case(name)
    tree = _tree(stl, torch, items)
    before = _content(torch, tree, max(len(items), 1))
    ans = GM.Answer(items, requests)
    _check(ans, _get(stl, torch, tree, requests, modes, max_nodes=ans.total))
    _check(ans, _get(stl, torch, tree, requests, modes, max_nodes=ans.total + 7, ids=False, meta=False, leaves=False,
                     counts=False))
    assert _content(torch, tree, max(len(items), 1)) == before
    tree.close()


# ---- 2. generated requests against random trees; FAT rows are nodes of the fetch pack against none ----
@pytest.mark.parametrize("n_items", [300, 131073])
def test_random_trees(stl, torch_cuda, n_items):
    torch = torch_cuda
    items = _random_items(n_items, 60 + n_items)
    tree = _tree(stl, torch, items, n_items + 3)
    requests = GM.requests_for(items, np.random.default_rng(61), 1000)
    nodes = NM.nodes_closed(items)
    ans = GM.Answer(items, requests, nodes=nodes)
    assert {GM.INNER, GM.LEAF, GM.ABSENT, GM.INVALID, GM.OTHER_LEAF} <= set(ans.status)
    g = _get(stl, torch, tree, requests, max_nodes=ans.total)
    _check(ans, g)
    pack = tree.fetch_pack_device(None, max_nodes=len(nodes) + 1)
    torch.cuda.synchronize()
    assert pack.rows() == len(nodes)
    by_hash = dict(zip((h.tobytes() for h in pack.hash[:pack.rows()].cpu().numpy()),
                       pack.body[:pack.rows()].cpu().numpy()))
    out = g.read()
    for i, (nid, depth, mode) in enumerate(requests):
        if mode != GM.FAT:
            continue
        for r in range(ans.first[i], ans.first[i] + ans.rows[i]):
            assert out[6][r].tobytes() == by_hash[out[5][r].tobytes()].tobytes()
    tree.close()


# ---- 3. more than 128 nodes a depth in one tile, with and without tasks ----
def test_one_bucket(stl, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(62)
    keys = rng.integers(0, 256, (40000, 32), dtype=np.uint8)
    keys[:, 0], keys[:, 1] = 0xC3, 0x5A
    keys = np.unique(keys, axis=0)
    leaves = rng.integers(0, 256, keys.shape, dtype=np.uint8)
    items = {k.tobytes(): v.tobytes() for k, v in zip(keys, leaves)}
    nodes = NM.nodes_closed(items)
    assert np.bincount([d for d, _ in nodes], minlength=64).max() > 128
    tree = _tree(stl, torch, items)
    requests = GM.requests_for(items, rng, 300)
    ans = GM.Answer(items, requests, nodes=nodes)
    assert ans.counts[4] == 1 and ans.counts[5] == len(items) and 0 < ans.counts[6] < len(nodes)
    _check(ans, _get(stl, torch, tree, requests, max_nodes=ans.total))
    tree.close()


# ---- 4. capacities ----
def test_capacities(stl, torch_cuda):
    torch = torch_cuda
    items = _random_items(300, 63)
    for cap in (8, 13):  # a full tree
        part = dict(list(items.items())[:cap])
        tree = _tree(stl, torch, part, cap)
        requests = GM.requests_for(part, np.random.default_rng(cap), 60)
        ans = GM.Answer(part, requests)
        _check(ans, _get(stl, torch, tree, requests, max_nodes=ans.total))
        tree.close()
    # a host bound above the count: deletes leave it loose
    tree = _tree(stl, torch, items, 1000)
    gone = list(items)[:100]
    k = np.frombuffer(b"".join(gone), np.uint8).reshape(-1, 32)
    tree.apply_device(_dev(torch, k), None, torch.ones(100, dtype=torch.uint8, device="cuda"))
    left = {key: v for key, v in items.items() if key not in set(gone)}
    requests = GM.requests_for(left, np.random.default_rng(64), 200) + [(key, 0, GM.PATH) for key in gone[:20]]
    ans = GM.Answer(left, requests)
    _check(ans, _get(stl, torch, tree, requests, max_nodes=ans.total))
    tree.close()


# ---- 5. overflow, no request, the host form ----
def test_overflow_no_request_and_host_form(stl, torch_cuda):
    torch = torch_cuda
    items, requests, _ = GM.case("parent_child")
    more, more_requests, _ = GM.case("pair63")
    tree, deep = _tree(stl, torch, items), _tree(stl, torch, more)
    for t, it, rq in ((tree, items, requests), (deep, more, more_requests)):
        nodes = NM.nodes_closed(it)
        full = GM.Answer(it, rq, nodes=nodes)
        middle = full.first[1] + max(full.rows[1] // 2, 1)
        for room in (0, full.total - 1, middle):
            _check(GM.Answer(it, rq, max_nodes=room, nodes=nodes), _get(stl, torch, t, rq, max_nodes=room))
        # the host form, with room and without
        rid, rdepth, rmode = GM.request_arrays(rq)
        for room in (full.total + 2, 5, 0):
            a = t.get_nodes(rid, rdepth, rmode, max_nodes=room)
            ans = GM.Answer(it, rq, max_nodes=room, nodes=nodes)
            GM.check_outputs(ans, a.status, a.first, a.rows, a.leaf_key, a.leaf_hash, a.nodes.hash, a.nodes.body,
                             a.nodes.ids, a.nodes.meta, a.nodes.count, a.counts)
        a = t.get_nodes(rid, rdepth, None, max_nodes=8, node_ids=False, meta=False, leaves=False)
        ans = GM.Answer(it, [(i, d, GM.FAT) for i, d, _ in rq], max_nodes=8, nodes=nodes)
        GM.check_outputs(ans, a.status, a.first, a.rows, None, None, a.nodes.hash, a.nodes.body, None, None,
                         a.nodes.count, a.counts)
    # no request: a count of zero and zero counts, nothing else
    g = _get(stl, torch, tree, [], max_nodes=4)
    out = g.read()
    assert out[9] == 0 and out[10] == [0] * 8
    a = tree.get_nodes(np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8), max_nodes=4)
    assert a.nodes.count == 0 and a.counts == [0] * 8
    # the wrapper's device form
    rid, rdepth, rmode = GM.request_arrays(requests)
    a = tree.get_nodes_device(_dev(torch, rid), _dev(torch, rdepth), _dev(torch, rmode), max_nodes=64, counts=True)
    torch.cuda.synchronize()
    ans = GM.Answer(items, requests, max_nodes=64)
    c = lambda t: t.cpu().numpy()  # noqa: E731
    GM.check_outputs(ans, c(a.status), c(a.first), c(a.rows), c(a.leaf_key), c(a.leaf_hash), c(a.nodes.hash),
                     c(a.nodes.body), c(a.nodes.ids), c(a.nodes.meta), int(a.nodes.count.item()), c(a.counts))
    tree.close(), deep.close()


# ---- 6. read-only, side by side ----
def test_two_calls_on_two_streams_leave_the_tree_alone(stl, torch_cuda):
    torch = torch_cuda
    items = _random_items(300, 65)
    other = dict(list(items.items())[:250])
    tree, second = _tree(stl, torch, items, 400), _tree(stl, torch, other, 350)
    probes = _dev(torch, np.frombuffer(b"".join(list(items)[:200]), np.uint8).reshape(-1, 32))
    requests = GM.requests_for(items, np.random.default_rng(66), 200)
    ans = GM.Answer(items, requests)
    before = _content(torch, tree, 400)
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a = _get(stl, torch, tree, requests, max_nodes=ans.total, stream=s1)  # enqueued back to back, no wait between
    b = _get(stl, torch, tree, requests, max_nodes=ans.total, stream=s2)
    words = tree.lookup_device(probes, stream=s3)
    diff = tree.compare_device(second, 100, stream=s3)
    _check(ans, a)
    _check(ans, b)
    assert int(diff.counts[0]) == 50
    assert np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")[:200].all()
    assert _content(torch, tree, 400) == before
    tree.close(), second.close()


# ---- 7. the failure contract ----
@pytest.mark.parametrize("form", ["device", "host"])
def test_fault_injection(stl, torch_cuda, form):
    """Every HIP call of one call failed in turn (at the API boundary: no device
    fault): the call returns < 0, the count words keep their guard value, the
    tree is unchanged, and the same call afterwards gives the model's answer."""
    from stellard_amd import _native as N
    torch = torch_cuda
    items, requests, _ = GM.case("all_modes")
    tree = _tree(stl, torch, items)
    ans = GM.Answer(items, requests)
    rid, rdepth, rmode = GM.request_arrays(requests)
    before = _content(torch, tree, len(items))
    stream = torch.cuda.Stream()  # a fresh context: the first call also allocates
    failed, kk = 0, 0
    try:
        while True:
            assert kk < 400, "the countdown never ran out"
            g = Guarded(stl, torch, len(requests), ans.total)
            inputs = (_dev(torch, rid), _dev(torch, rdepth), _dev(torch, rmode))
            a = None
            torch.cuda.synchronize()
            stl.debug_fault_after(kk)
            kk += 1
            try:
                if form == "host":
                    a = tree.get_nodes(rid, rdepth, rmode, max_nodes=ans.total)
                else:
                    N.check(g.call(tree, *inputs, stream=stream), "stl_shamap_tree_get_nodes_device")
                    torch.cuda.synchronize()
            except N.StlError as e:
                assert e.rc < 0
                failed += 1
                stl.debug_fault_after(-1)
                torch.cuda.synchronize()
                assert g.untouched(), kk
                assert _content(torch, tree, len(items)) == before, kk
                continue
            stl.debug_fault_after(-1)
            if form == "host":
                GM.check_outputs(ans, a.status, a.first, a.rows, a.leaf_key, a.leaf_hash, a.nodes.hash, a.nodes.body,
                                 a.nodes.ids, a.nodes.meta, a.nodes.count, a.counts)
            else:
                _check(ans, g)
            break  # no call left to fail
    finally:
        stl.debug_fault_after(-1)
    torch.cuda.synchronize()
    assert failed == kk - 1
    # the memset, three scans, ranges, tasks, buckets, gather, neighbours, 60 x 2 level launches, five top
    # launches and the finish
    assert failed >= 1 + 3 + 5 + 120 + 5 + 1, (form, failed)
    assert _content(torch, tree, len(items)) == before
    tree.close()


def test_handles_that_are_not_live(stl, torch_cuda):
    from stellard_amd import _native as N
    torch = torch_cuda
    dead = stl.ShamapTree(16)
    h = dead.handle.value
    dead.close()

    class Dead:
        handle = ctypes.c_void_p(h)

    items, requests, _ = GM.case("one_key")
    rid, rdepth, rmode = GM.request_arrays(requests)
    g = Guarded(stl, torch, len(requests), 4)
    assert g.call(Dead, _dev(torch, rid), _dev(torch, rdepth), _dev(torch, rmode)) == N.STL_EINVAL
    a = np.zeros((len(requests), 32), np.uint8)
    out = stl.HostNodes(4).struct()
    assert N.load().stl_shamap_tree_get_nodes(
        h, rid.ctypes.data, rdepth.ctypes.data, None, len(requests), a.ctypes.data, a.ctypes.data, a.ctypes.data, None,
        None, ctypes.byref(out), None) == N.STL_EINVAL
    torch.cuda.synchronize()
    assert g.untouched() and not a.any()


# ---- 8. phase timing and the fixture ----
def test_phase_timing_counts_the_call(stl, torch_cuda):
    torch = torch_cuda
    items, requests, _ = GM.case("all_modes")
    tree = _tree(stl, torch, items)
    torch.cuda.synchronize()
    stl.reset_stats()
    stl.set_phase_timing(True)
    try:
        _get(stl, torch, tree, requests).read()
        st = stl.get_stats()
    finally:
        stl.set_phase_timing(False)
    ph = list(st["phase_ns"].values())
    assert st["phase_chunks"] == 1 and all(v > 0 for v in ph[:3])
    tree.close()


def test_golden_answers(stl, torch_cuda):
    torch = torch_cuda
    with open(GM.GOLDEN) as f:
        doc = json.load(f)
    for a in doc["answers"]:
        items = {bytes.fromhex(k): bytes.fromhex(v) for k, v in a["items"]}
        requests = [(bytes.fromhex(i), d, m) for i, d, m in a["requests"]]
        tree = _tree(stl, torch, items)
        assert tree.root_device()[0].cpu().numpy().tobytes().hex() == a["root"]
        out = _get(stl, torch, tree, requests, max_nodes=len(a["nodes"])).read()
        assert [int(x) for x in out[0]] == a["status"] and [int(x) for x in out[2]] == a["rows"]
        assert [bytes(k).hex() for k in out[3]] == a["leaf_key"] and out[10] == a["counts"]
        got = [{"depth": int(out[8][i]) & 0xFF, "id": bytes(out[7][i]).hex(), "hash": bytes(out[5][i]).hex(),
                "leaf_mask": (int(out[8][i]) & 0xFFFFFFFF) >> 16} for i in range(len(a["nodes"]))]
        assert got == a["nodes"]
        tree.close()
