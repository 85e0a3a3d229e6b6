"""GPU tests of the node-storing calls (stl_shamap_nodes*,
stl_shamap_tree_apply_nodes*): the rows a call writes, read as a dict keyed by
(depth, id) and never by position, equal the model of tests/shamap_nodes_py.py;
root and counts equal the model's and the non-storing calls'; every output sits
in a guarded buffer -- a guard row behind row max_nodes of each array, guard
words beside the count.

Run on an MI355X:  python -u -m pytest tests/test_gpu_shamap_nodes.py -m gpu -x -v
"""
import numpy as np
import pytest

from tests import shamap_nodes_py as NM
from tests import shamap_py as SM
from tests import shamap_tree_py as TM

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_WORD = 0x5A5A5A5A
# the level kernel's constants (stellard_amd/csrc/stl_shamap.hip), for the span arithmetic of the large case
LEVEL_BLOCK, LEVEL_TILE_NODES, LEVEL_GRID, LEVEL_SPANS_WANTED, LEVEL_SPAN_CHUNKS_MAX = 256, 128, 1024, 512, 16


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


def _leaves(keys, seed):
    return np.random.default_rng(seed).integers(0, 256, np.asarray(keys).shape, dtype=np.uint8)


def _k(*rows):
    return np.ascontiguousarray(np.stack([np.frombuffer(bytes(r), np.uint8) for r in rows]))


def _partner(key, shared, rng):
    """A key that shares exactly `shared` nibbles with key."""
    hx = bytes(key).hex()
    other = "%x" % (int(hx[shared], 16) ^ (1 + int(rng.integers(0, 15))))
    tail = rng.integers(0, 256, 32, dtype=np.uint8).tobytes().hex()[shared + 1:]
    return np.frombuffer(bytes.fromhex(hx[:shared] + other + tail), np.uint8).copy()


class Guarded:
    """The outputs of one call in guarded device buffers: max_nodes rows of
    each array and a guard row behind them, root and counts between guard rows,
    the count between guard words."""

    def __init__(self, torch, stl, max_nodes, count_words, ids=True, meta=True):
        self.torch, self.max_nodes = torch, max_nodes
        u8 = lambda w: torch.full((max_nodes + 1, w), GUARD, dtype=torch.uint8, device="cuda")  # noqa: E731
        self.hash, self.body = u8(32), u8(512)
        self.ids = u8(32) if ids else None
        self.meta = torch.full((max_nodes + 1,), GUARD_WORD, dtype=torch.int32, device="cuda") if meta else None
        self.cnt = torch.full((3,), GUARD_WORD, dtype=torch.int32, device="cuda")
        self.root = torch.full((3, 32), GUARD, dtype=torch.uint8, device="cuda")
        self.counts = torch.full((3 * count_words,), GUARD_WORD, dtype=torch.int32, device="cuda")
        self.words = count_words
        self.nodes = stl.DeviceNodes(max_nodes, ids=self.ids if ids else False, meta=self.meta if meta else False,
                                     hash=self.hash, body=self.body, count=self.cnt[1:2])

    def kwargs(self):
        return dict(nodes=self.nodes, out_root=self.root[1:2], counts=self.counts[self.words:2 * self.words])

    def untouched(self):
        """Nothing but guard bytes anywhere: what a refused call leaves."""
        t = [self.hash, self.body, self.root] + [x for x in (self.ids,) if x is not None]
        w = [self.cnt, self.counts] + [x for x in (self.meta,) if x is not None]
        return all(bool((x == GUARD).all()) for x in t) and all(bool((x == GUARD_WORD).all()) for x in w)

    def count_unwritten(self):
        return bool((self.cnt == GUARD_WORD).all()) and bool((self.root == GUARD).all()) and \
            bool((self.counts == GUARD_WORD).all())

    def read(self):
        """After the device is idle: the guards are intact -> (root, counts,
        count, the written rows as arrays (depth, ids, hash, body, mask) or,
        without ids or meta, the set of (hash, body))."""
        m, w = self.max_nodes, self.words
        assert (self.root[0] == GUARD).all() and (self.root[2] == GUARD).all(), "guards beside the root overwritten"
        assert (self.counts[:w] == GUARD_WORD).all() and (self.counts[2 * w:] == GUARD_WORD).all()
        assert int(self.cnt[0]) == GUARD_WORD and int(self.cnt[2]) == GUARD_WORD, "guards beside the count overwritten"
        for t in (self.hash, self.body, self.ids):
            assert t is None or (t[m] == GUARD).all(), "the guard row behind row max_nodes overwritten"
        assert self.meta is None or int(self.meta[m]) == GUARD_WORD
        count = int(self.cnt[1]) & 0xFFFFFFFF
        rows = min(count, m)
        root = self.root[1].cpu().numpy().tobytes()
        counts = [int(x) for x in self.counts[w:2 * w].cpu().numpy()]
        h, b = self.hash[:rows].cpu().numpy(), self.body[:rows].cpu().numpy()
        if self.ids is None or self.meta is None:
            got = {(h[j].tobytes(), b[j].tobytes()) for j in range(rows)}
            assert len(got) == rows
            return root, counts, count, got
        meta = self.meta[:rows].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        assert ((meta >> 8) & 0xFF == 0).all(), "bits 8-15 of a meta word are set"
        return root, counts, count, (meta & 0xFF, self.ids[:rows].cpu().numpy(), h, b, meta >> 16)


def run_set(torch, stl, keys, leaves=None, select=None, max_nodes=None, ids=True, meta=True, stream=None):
    keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
    n = keys.shape[0]
    if max_nodes is None:
        max_nodes = 63 * max(n - 1, 0) + 1
    g = Guarded(torch, stl, max_nodes, 4, ids, meta)
    k = _dev(torch, keys) if n else torch.zeros((0, 32), dtype=torch.uint8, device="cuda")
    sel = None
    if select is not None:
        words = np.zeros((n + 63) // 64 * 8, np.uint8)
        packed = np.packbits(np.asarray(select, bool), bitorder="little")
        words[:packed.size] = packed
        sel = _dev(torch, words.view(np.int64))
    torch.cuda.synchronize()
    stl.shamap_nodes_device(k, _dev(torch, leaves), sel, stream=stream, **g.kwargs())
    torch.cuda.synchronize()
    return g.read()


def check_set(torch, stl, keys, leaves=None, select=None, **kw):
    """One storing call against the model -> (root, counts)."""
    root, counts, count, got = run_set(torch, stl, keys, leaves, select, **kw)
    assert (root, counts) == SM.model(keys, leaves, select)
    want = NM.nodes(keys, leaves, select)
    assert count == counts[2] == len(want)
    if isinstance(got, set):
        assert got == {(v[0], v[1]) for v in want.values()}
    else:
        assert NM.as_dict(*got) == want
    return root, counts


# ---- 1. tiny maps ----
def test_tiny_maps(stl, torch_cuda):
    torch = torch_cuda
    assert run_set(torch, stl, np.zeros((0, 32), np.uint8), max_nodes=4)[:3] == (SM.ZERO, [0, 0, 0, 0], 0)
    for n in (1, 2, 3):
        check_set(torch, stl, SM.case_keys(f"random{n}", 10 + n), _leaves(np.zeros((n, 32)), 20 + n))
    _, counts = check_set(torch, stl, SM.case_keys("deepest", 14))  # two keys parting at nibble 63: the chain of 64
    assert counts == [2, 0, 64, 63]
    chain = np.zeros((5, 32), np.uint8)
    chain[:, 31] = np.arange(5)
    assert check_set(torch, stl, chain, _leaves(chain, 15))[1] == [5, 0, 64, 63]
    # nothing selected: the empty map through the kernels
    assert run_set(torch, stl, SM.case_keys("random3", 16), select=np.zeros(3, bool))[:3] == (SM.ZERO, [0, 0, 0, 0], 0)


# ---- 2. keys equal in their first 8 / 16 / 24 bytes; 3. select and duplicates; 4. leaf hashes; 5. no id, no meta ----
def test_multiword_select_duplicates_and_optional_arrays(stl, torch_cuda):
    torch = torch_cuda
    keys = SM.case_keys("multiword", 30)
    check_set(torch, stl, keys)
    check_set(torch, stl, keys, _leaves(keys, 31))
    dups = SM.case_keys("dups1000", 32)
    lh = _leaves(dups, 33)
    sel = np.random.default_rng(34).random(1000) < 0.6
    _, c = check_set(torch, stl, dups, lh, sel)
    assert c[1] > 0
    check_set(torch, stl, dups, None, sel)
    check_set(torch, stl, dups, lh)
    for ids, meta in ((False, True), (True, False), (False, False)):
        check_set(torch, stl, dups, lh, sel, ids=ids, meta=meta)


# ---- 6. tile and span edges of the level kernel ----
@pytest.mark.parametrize("shape", ["random255", "random256", "random257", "dense129", "random131073"])
def test_tile_and_span_edges(stl, torch_cuda, shape):
    torch = torch_cuda
    if shape == "dense129":
        # 129 nodes of one depth within one span's reach: 129 pairs that part at nibble 63 sort first (four
        # zero bytes in front), 66,000 random keys behind them.  Depth 63 then holds 129 nodes in 259 chunks,
        # so a span is two chunks (259 * 1 / 129), and the first span meets 128 nodes in chunk 0 and one more
        # in chunk 1: the tile of 128 is flushed in the middle of the span.
        rng = np.random.default_rng(60)
        head = rng.integers(0, 256, 32, dtype=np.uint8)
        head[:4] = 0
        keys = np.repeat(head[None], 258, axis=0)
        pair = np.arange(258) // 2
        keys[:, 5] = pair >> 4
        keys[:, 6] = (pair & 15) << 4 | (keys[:, 6] & 15)
        keys[:, 31] = (keys[:, 31] & 0xF0) | (np.arange(258) % 2)
        keys = np.concatenate([keys, SM.case_keys("random66000", 61)])
        keys = keys[rng.permutation(keys.shape[0])]
        assert sorted(k.tobytes() for k in keys)[257][:4] == bytes(4)  # the pairs are the first 258 positions
        chunks = (keys.shape[0] + LEVEL_BLOCK - 1) // LEVEL_BLOCK
        assert chunks * 1 // 129 == 2 <= LEVEL_SPAN_CHUNKS_MAX
    else:
        keys = SM.case_keys(shape, 62)
    leaves = _leaves(keys, 63)
    root, counts, count, got = run_set(torch, stl, keys, leaves, max_nodes=4 * keys.shape[0] + 64 * 130)
    assert (root, counts) == SM.model(keys, leaves)
    assert count == counts[2]
    if shape == "dense129":
        assert int((got[0] == 63).sum()) == 129
    assert NM.same_nodes(got, NM.nodes_closed_arrays(SM.the_set(keys, leaves)[0]))


# ---- 7. more nodes at one depth than one pass of the grid takes ----
def test_more_than_one_span_per_workgroup(stl, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(70)
    pairs = 132000
    prefix = rng.permutation(1 << 20)[:pairs].astype(np.int64)  # distinct 5-nibble prefixes
    keys = rng.integers(0, 256, (2 * pairs, 32), dtype=np.uint8)
    nib = rng.integers(0, 16, pairs)
    other = nib ^ rng.integers(1, 16, pairs)
    for half, sixth in ((0, nib), (1, other)):  # a pair shares exactly five nibbles
        keys[half::2, 0] = prefix >> 12
        keys[half::2, 1] = (prefix >> 4) & 0xFF
        keys[half::2, 2] = ((prefix & 15) << 4) | sixth
    keys = keys[rng.permutation(2 * pairs)]
    want = NM.nodes_closed_arrays(SM.the_set(keys)[0])
    at5 = int((want[0] == 5).sum())
    assert at5 == pairs > LEVEL_GRID * LEVEL_TILE_NODES
    # the kernel's span arithmetic at depth 5: one chunk per span, more spans than workgroups
    chunks = (2 * pairs + LEVEL_BLOCK - 1) // LEVEL_BLOCK
    per = max(1, min(LEVEL_SPAN_CHUNKS_MAX,
                     chunks * min(LEVEL_TILE_NODES, -(-at5 // LEVEL_SPANS_WANTED)) // at5))
    assert -(-chunks // per) > LEVEL_GRID
    root, counts, count, got = run_set(torch, stl, keys, max_nodes=len(want[0]) + 5)
    assert count == counts[2] == len(want[0]) and counts[0] == 2 * pairs and 190000 < count < 210000
    assert NM.same_nodes(got, want)
    plain, pc = stl.shamap_root_device(_dev(torch, keys), counts=True)
    torch.cuda.synchronize()
    assert plain[0].cpu().numpy().tobytes() == root and [int(x) for x in pc.cpu()] == counts


# ---- 8. overflow ----
def test_overflow(stl, torch_cuda):
    torch = torch_cuda
    keys = SM.case_keys("cluster3000_40_9", 80)
    leaves = _leaves(keys, 81)
    want = NM.nodes(keys, leaves)
    full = len(want)
    assert full > 3 * LEVEL_TILE_NODES
    for max_nodes in (0, 1, full - 1, full):
        root, counts, count, got = run_set(torch, stl, keys, leaves, max_nodes=max_nodes)
        assert (root, counts) == SM.model(keys, leaves) and count == full
        got = NM.as_dict(*got)  # distinct nodes
        assert len(got) == min(max_nodes, full) and all(want[k] == v for k, v in got.items())
    # the host form: the same rows come back, and only min(count, max_nodes) of them
    for max_nodes in (0, full // 2, full + 3):
        root, counts, nodes = stl.shamap_nodes(keys, leaves, max_nodes=max_nodes)
        assert (root, counts) == SM.model(keys, leaves) and nodes.count == full
        got = NM.rows_as_dict(nodes.rows(), nodes.hash, nodes.body, nodes.ids, nodes.meta)
        assert len(got) == min(max_nodes, full) and all(want[k] == v for k, v in got.items())
        assert not nodes.hash[nodes.rows():].any() and not nodes.body[nodes.rows():].any()
    sel = np.random.default_rng(82).random(3000) < 0.5
    root, counts, nodes = stl.shamap_nodes(keys, None, sel, max_nodes=full, ids=False, meta=False)
    assert (root, counts) == SM.model(keys, None, sel) and nodes.count == counts[2]
    assert stl.shamap_nodes(np.zeros((0, 32), np.uint8), max_nodes=2)[:2] == (SM.ZERO, [0, 0, 0, 0])


# ---- 9. the tree ----
class Rig:
    """A tree on the device and its model, stepped together through the storing apply."""

    def __init__(self, torch, stl, capacity, stream=None):
        self.torch, self.stl, self.cap, self.stream = torch, stl, capacity, stream
        self.tree = stl.ShamapTree(capacity)
        self.m = TM.Model()

    def content(self):
        torch = self.torch
        k = torch.zeros((self.cap, 32), dtype=torch.uint8, device="cuda")
        l = torch.zeros((self.cap, 32), dtype=torch.uint8, device="cuda")
        items = self.tree.export_device(k, l, stream=self.stream)
        torch.cuda.synchronize()
        m = int(items[0])
        return k[:m], l[:m]

    def check_content(self, want_root):
        k, l = self.content()
        wk, wl = self.m.content()
        assert np.array_equal(k.cpu().numpy(), wk) and np.array_equal(l.cpu().numpy(), wl)
        r = self.tree.root_device(stream=self.stream)
        self.torch.cuda.synchronize()
        assert r[0].cpu().numpy().tobytes() == want_root

    def apply(self, keys, leaves=None, ops=None, max_nodes=None):
        torch = self.torch
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
        if max_nodes is None:
            max_nodes = 63 * max(len(self.m.items) + keys.shape[0] - 1, 0) + 1
        g = Guarded(torch, self.stl, max_nodes, 8)
        k = _dev(torch, keys) if keys.shape[0] else torch.zeros((0, 32), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.last = g
        self.tree.apply_nodes_device(k, _dev(torch, leaves), _dev(torch, ops), stream=self.stream, **g.kwargs())
        torch.cuda.synchronize()
        return g.read()

    def step(self, keys, leaves=None, ops=None, max_nodes=None):
        """One storing apply against the model: E, root, counts, content -> (counts, E)."""
        want_root, want_counts = self.m.apply(keys, leaves, ops)
        e = NM.emitted(self.m.items, keys) if len(keys) else {}
        root, counts, count, got = self.apply(keys, leaves, ops, max_nodes)
        assert counts == want_counts, (counts, want_counts)
        assert root == want_root and count == len(e)
        got = NM.as_dict(*got)
        if max_nodes is None:
            assert got == e
        else:
            assert len(got) == min(max_nodes, len(e)) and all(e[k] == v for k, v in got.items())
        self.check_content(want_root)
        return counts, e

    def close(self):
        self.tree.close()


def test_tree_load_and_mixed_sequence(stl, torch_cuda):
    rng = np.random.default_rng(90)
    rig = Rig(torch_cuda, stl, 6000)
    assert rig.step(np.zeros((0, 32), np.uint8))[1] == {}  # n == 0 on the empty tree
    keys = SM.case_keys("random3000", 91)
    counts, e = rig.step(keys, _leaves(keys, 92))  # the load of an empty tree: every inner node
    assert e == NM.nodes_closed(rig.m.items)
    seen = [0] * 8
    for rows in (1, 37, 300, 700):
        old = NM.hashes_of(NM.nodes_closed(rig.m.items))
        counts, e = rig.step(*TM._mixed_batch(rng, rig.m.items, rows))
        new = NM.nodes_closed(rig.m.items)
        assert {k for k, v in new.items() if v[0] not in old} <= set(e)  # the guarantee
        seen = [a + b for a, b in zip(seen, counts)]
    assert all(seen[i] > 0 for i in range(1, 8)), seen
    root, counts, count, _ = rig.apply(np.zeros((0, 32), np.uint8), max_nodes=3)  # n == 0: the root, no node
    assert (root, counts, count) == (rig.m.root(), [len(rig.m.items)] + [0] * 7, 0)
    # deletes of absent keys: dirty buckets, nothing changed, their nodes stored all the same
    gone = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    before = rig.m.root()
    counts, e = rig.step(gone, None, np.ones(40, np.uint8))
    assert counts[4] == 40 and counts[6] > 0 and e and rig.m.root() == before
    # overflow through the tree's call
    batch = TM._mixed_batch(rng, rig.m.items, 200)
    rig.step(*batch, max_nodes=7)
    rig.close()


def test_tree_bucket_edges(stl, torch_cuda):
    rng = np.random.default_rng(100)
    rig = Rig(torch_cuda, stl, 700)
    dele = np.array([1], np.uint8)
    for shared in (3, 4, 63, 0, 5):  # 3: the pair's node is the top kernel's; 4: the level kernel's
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        b = _partner(a, shared, rng)
        rig.step(_k(a), _k(_leaves(a, shared)))
        _, e = rig.step(_k(b))
        assert max(d for d, _ in e) == shared
        _, e = rig.step(_k(a), None, dele)  # the 2 -> 1 collapse: the chain is gone
        assert all(d < min(shared, 4) or d == 0 for d, _ in e)
        rig.step(_k(b), None, dele)  # a delete that empties the bucket
    assert rig.m.root() == SM.ZERO
    # keys on both sides of a bucket boundary: the last key of bucket 0x1233 and the first of 0x1234
    lo, hi = np.full(32, 0xFF, np.uint8), np.zeros(32, np.uint8)
    lo[:2], hi[:2] = (0x12, 0x33), (0x12, 0x34)
    near = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    near[:3, :2], near[3:, :2] = (0x12, 0x33), (0x12, 0x34)
    rig.step(np.concatenate([_k(lo, hi), near]), _leaves(np.zeros((8, 32)), 101))
    counts, e = rig.step(_k(hi), None, dele)
    assert counts[6] == 1 and not any(d >= 4 and nid[:2] == b"\x12\x33" for d, nid in e)
    rig.step(_k(lo, hi), _leaves(np.zeros((2, 32)), 102))
    # one bucket holding everything
    one = np.unique(SM.case_keys("cluster600_1_50", 103), axis=0)
    rig2 = Rig(torch_cuda, stl, one.shape[0] + 4)
    counts, _ = rig2.step(one[:400], _leaves(one[:400], 104))
    assert counts[6] == 1 and counts[7] == 400
    rig2.step(np.concatenate([one[400:], one[:50]]), None,
              np.concatenate([np.zeros(one.shape[0] - 400, np.uint8), np.ones(50, np.uint8)]))
    rig.close()
    rig2.close()


def test_tree_capacity(stl, torch_cuda):
    from stellard_amd import _native as N
    torch = torch_cuda
    rig = Rig(torch, stl, 1000)
    keys = SM.case_keys("random2100", 110)
    rig.step(keys[:600], _leaves(keys[:600], 111))
    # the bound (600 + 600) no longer admits the batch: the call waits once and goes through
    counts, _ = rig.step(keys[:600], _leaves(keys[:600], 112))
    assert counts[:5] == [600, 0, 600, 0, 0]
    rig.step(keys[600:1000])  # exactly full
    with pytest.raises(N.StlError) as err:
        rig.apply(keys[1000:1001])
    assert err.value.rc == N.STL_ENOMEM
    torch.cuda.synchronize()
    assert rig.last.untouched()  # root, counts, the count and the arrays' guard bytes are as before
    rig.check_content(rig.m.root())
    with pytest.raises(N.StlError) as err:
        rig.apply(keys[:1001])
    assert err.value.rc == N.STL_EINVAL and rig.last.untouched()
    counts, _ = rig.step(keys[:10], None, np.ones(10, np.uint8))  # a full tree still takes deletes
    assert counts[:5] == [990, 0, 0, 10, 0]
    rig.close()


# ---- 10. the set call over a tree's export; 11. the non-storing calls agree ----
def test_export_union_and_parity_with_the_plain_calls(stl, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(120)
    rig = Rig(torch, stl, 9000)
    plain = stl.ShamapTree(9000)
    keys = SM.case_keys("cluster5000_300_6", 121)
    batches = [(keys, _leaves(keys, 122), None)]
    rig.step(*batches[0])
    for rows in (50, 600):
        batches.append(TM._mixed_batch(rng, rig.m.items, rows))
        rig.step(*batches[-1])
    m2 = TM.Model()
    for b in batches:  # the plain apply on the same input: the same root and counts
        r, c = plain.apply_device(*[_dev(torch, x) for x in b], counts=True)
        torch.cuda.synchronize()
        assert (r[0].cpu().numpy().tobytes(), [int(x) for x in c.cpu()]) == m2.apply(*b)
    assert m2.root() == rig.m.root()
    k, l = rig.content()
    g = Guarded(torch, stl, 63 * 9000, 4)
    stl.shamap_nodes_device(k.contiguous(), l.contiguous(), **g.kwargs())
    torch.cuda.synchronize()
    root, counts, count, got = g.read()
    assert root == rig.m.root() and count == counts[2]
    assert NM.as_dict(*got) == NM.nodes_closed(rig.m.items)  # the union of everything the tree holds
    r, c = stl.shamap_root_device(k.contiguous(), l.contiguous(), counts=True)
    torch.cuda.synchronize()
    assert (r[0].cpu().numpy().tobytes(), [int(x) for x in c.cpu()]) == (root, counts)
    rig.close()
    plain.close()


# ---- 12. injected errors ----
def test_fault_injection(stl, torch_cuda):
    """Every HIP call of one storing set call and of one storing apply failed
    in turn (at the API boundary: no device fault): the call returns < 0, the
    count, root and counts are not written, the tree is unchanged, and the same
    call made again gives the model's result."""
    from stellard_amd import _native as N
    torch = torch_cuda
    rng = np.random.default_rng(130)
    stream = torch.cuda.Stream()  # a fresh context: the first call also allocates
    keys = SM.case_keys("random300", 131)
    leaves = _leaves(keys, 132)
    want = NM.nodes(keys, leaves)
    dk, dl = _dev(torch, keys), _dev(torch, leaves)
    failed = kk = 0
    try:
        while True:
            assert kk < 200, "the countdown never ran out"
            g = Guarded(torch, stl, len(want), 4)
            torch.cuda.synchronize()
            stl.debug_fault_after(kk)
            kk += 1
            try:
                stl.shamap_nodes_device(dk, dl, stream=stream, **g.kwargs())
            except N.StlError as e:
                assert e.rc < 0
                failed += 1
                stl.debug_fault_after(-1)
                torch.cuda.synchronize()
                assert g.count_unwritten(), kk
                continue
            stl.debug_fault_after(-1)
            torch.cuda.synchronize()
            root, counts, count, got = g.read()
            assert (root, counts) == SM.model(keys, leaves) and NM.as_dict(*got) == want
            break
    finally:
        stl.debug_fault_after(-1)
    assert failed == kk - 1 and failed >= 70, failed  # the memset, the sort, heads, scan, 64 levels, finish
    rig = Rig(torch, stl, 4000, stream=stream)
    rig.step(keys, leaves)
    failed = kk = 0
    try:
        while True:
            assert kk < 250, "the countdown never ran out"
            batch = TM._mixed_batch(rng, rig.m.items, 40)
            before = rig.m.root()
            torch.cuda.synchronize()
            stl.debug_fault_after(kk)
            kk += 1
            try:
                got = rig.apply(*batch)
            except N.StlError as e:
                assert e.rc < 0
                failed += 1
                stl.debug_fault_after(-1)
                torch.cuda.synchronize()
                assert rig.last.count_unwritten(), kk
                rig.check_content(before)
                rig.step(*batch)  # the same batch, clean
                continue
            stl.debug_fault_after(-1)
            want_root, want_counts = rig.m.apply(*batch)
            assert (got[0], got[1]) == (want_root, want_counts)
            assert NM.as_dict(*got[3]) == NM.emitted(rig.m.items, batch[0])
            rig.check_content(want_root)
            break
    finally:
        stl.debug_fault_after(-1)
    assert failed == kk - 1 and failed >= 88, failed
    rig.close()


# ---- 13. streams and two trees ----
def test_streams_and_two_trees(stl, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(140)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = Rig(torch, stl, 6000, stream=s1), Rig(torch, stl, 3000, stream=s2)
    ka, kb = SM.case_keys("random4097", 141), SM.case_keys("cluster2000_9_20", 142)
    a.step(ka, _leaves(ka, 143))
    b.step(kb)
    for rows in (64, 300):  # interleaved, each on its own stream
        a.step(*TM._mixed_batch(rng, a.m.items, rows))
        b.step(*TM._mixed_batch(rng, b.m.items, rows + 1))
    check_set(torch, stl, kb, _leaves(kb, 144), stream=s2)
    # the host form of the apply equals the model as well
    host, hm = stl.ShamapTree(6000), TM.Model()
    for bt in [(ka, _leaves(ka, 143), None)] + [TM._mixed_batch(rng, a.m.items, 200)]:
        want = hm.apply(*bt)
        e = NM.emitted(hm.items, bt[0])
        root, counts, nodes = host.apply_nodes(*bt, max_nodes=len(e) + 2)
        assert (root, counts) == want and nodes.count == len(e)
        assert NM.rows_as_dict(nodes.rows(), nodes.hash, nodes.body, nodes.ids, nodes.meta) == e
    root, counts, nodes = host.apply_nodes(np.zeros((0, 32), np.uint8), max_nodes=1)
    assert (root, counts[0], nodes.count) == (hm.root(), len(hm.items), 0)
    host.close()
    a.close()
    b.close()
