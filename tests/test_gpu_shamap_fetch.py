"""GPU tests of the fetch pack between two resident SHAMaps
(stl_shamap_tree_fetch_pack*): on guarded outputs the rows are, as a set of
nodes -- hash, body, ID and meta all compared -- the model of
tests/shamap_fetch_py.py: every inner node of want for which have holds no
inner node at the same ID with the same hash; the eight counts are the model's;
both trees are byte-equal to what they were.

Run on an MI355X:  python -u -m pytest tests/test_gpu_shamap_fetch.py -m gpu -x -v
"""
import json

import numpy as np
import pytest

from tests import shamap_fetch_py as FP
from tests import shamap_lookup_py as LM
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
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.shape[0] == 0:
        return torch.zeros(a.shape, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a).cuda()


def _tree(stl, torch, items, capacity=None):
    """A resident tree holding {key: leaf hash}, built by the existing apply."""
    t = stl.ShamapTree(capacity if capacity is not None else max(len(items), 1))
    if items:
        k, l = LM.arrays(items)
        t.apply_device(_dev(torch, k), _dev(torch, l))
    return t


class Guarded:
    """Output arrays of max_nodes rows with a guard row on either side, and guarded count words."""

    def __init__(self, stl, torch, max_nodes, ids=True, meta=True, counts=True):
        self.torch, self.max_nodes = torch, max_nodes
        rows = max(max_nodes, 1)
        u8 = lambda w: torch.full((rows + 2, w), GUARD, dtype=torch.uint8, device="cuda")  # noqa: E731
        self.hash, self.body = u8(32), u8(512)
        self.ids = u8(32) if ids else None
        self.meta = torch.full((rows + 2,), GUARD_WORD, dtype=torch.int32, device="cuda") if meta else None
        self.count = torch.full((3,), GUARD_WORD, dtype=torch.int32, device="cuda")
        self.counts = torch.full((24,), GUARD_WORD, dtype=torch.int32, device="cuda") if counts else None
        inner = lambda t: False if t is None else t[1:rows + 1]  # noqa: E731
        self.nodes = stl.DeviceNodes(max_nodes, ids=inner(self.ids), meta=inner(self.meta), hash=inner(self.hash),
                                     body=inner(self.body), count=self.count[1:2])

    def untouched(self):
        """Nothing at all was written: what a failed call must leave of the count words."""
        c = self.counts is None or bool((self.counts == GUARD_WORD).all())
        return c and bool((self.count == GUARD_WORD).all())

    def read(self):
        """Waits; checks every guard -> ({(depth, id): (hash, body, leaf mask)}, count, counts or None)."""
        torch, room = self.torch, self.max_nodes
        torch.cuda.synchronize()
        count = int(self.count[1])
        assert int(self.count[0]) == GUARD_WORD and int(self.count[2]) == GUARD_WORD
        rows = min(count, room)
        for t in (self.hash, self.body, self.ids):
            if t is not None:
                assert (t[0] == GUARD).all() and (t[rows + 1:] == GUARD).all(), "a store past the rows written"
        if self.meta is not None:
            assert int(self.meta[0]) == GUARD_WORD and (self.meta[rows + 1:] == GUARD_WORD).all()
        counts = None
        if self.counts is not None:
            assert (self.counts[:8] == GUARD_WORD).all() and (self.counts[16:] == GUARD_WORD).all()
            counts = [int(x) for x in self.counts[8:16].cpu()]
        got = None
        if self.ids is not None and self.meta is not None:
            got = NM.rows_as_dict(rows, self.hash[1:].cpu().numpy(), self.body[1:].cpu().numpy(),
                                  self.ids[1:].cpu().numpy(), self.meta[1:].cpu().numpy())
        return got, count, counts

    def arrays(self):
        """The rows written as shamap_nodes_py's tuple of arrays (depth, ids, hash, body, leaf mask)."""
        rows = min(int(self.count[1]), self.max_nodes)
        meta = self.meta[1:rows + 1].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        return (meta & 0xFF, self.ids[1:rows + 1].cpu().numpy(), self.hash[1:rows + 1].cpu().numpy(),
                self.body[1:rows + 1].cpu().numpy(), meta >> 16)


def _pack(stl, torch, want, have, max_nodes, stream=None, **kw):
    g = Guarded(stl, torch, max_nodes, **kw)
    torch.cuda.synchronize()
    want.fetch_pack_device(have, nodes=g.nodes, counts=g.counts[8:16] if g.counts is not None else False,
                           stream=stream)
    return g


def _content(torch, tree, rows):
    k = torch.full((rows + 1, 32), GUARD, dtype=torch.uint8, device="cuda")
    l = torch.full((rows + 1, 32), GUARD, dtype=torch.uint8, device="cuda")
    items = tree.export_device(k[:rows], l[:rows])
    r = tree.root_device()
    torch.cuda.synchronize()
    assert (k[rows] == GUARD).all() and (l[rows] == GUARD).all()
    m = int(items[0])
    return k[:m].cpu().numpy().tobytes(), l[:m].cpu().numpy().tobytes(), r[0].cpu().numpy().tobytes()


def _applied(items, keys, leaves, ops):
    """The content after a batch: the rows one after another, the last of equal keys counting."""
    out = dict(items)
    for i in range(len(keys)):
        k = keys[i].tobytes()
        if ops is not None and ops[i]:
            out.pop(k, None)
        else:
            out[k] = k if leaves is None else leaves[i].tobytes()
    return out


def _room(items):
    return 63 * max(len(items) - 1, 0) + 1


# ---- 1. the named pairs: trivial ones, the two ID cases, the bucket cases ----
@pytest.mark.parametrize("name", FP.PAIRS)
def test_named_pairs(stl, torch_cuda, name):
    torch = torch_cuda
    wi, hi = FP.pair(name)
    want, have = _tree(stl, torch, wi), _tree(stl, torch, hi)
    empty, twin = _tree(stl, torch, {}), _tree(stl, torch, wi, len(wi) + 5)
    before = _content(torch, want, max(len(wi), 1)), _content(torch, have, max(len(hi), 1))
    for hv_tree, hv in ((have, hi), (empty, {}), (None, None), (want, wi), (twin, wi)):
        pack = FP.pack_by_difference(wi, hv)
        got, count, counts = _pack(stl, torch, want, hv_tree, _room(wi)).read()
        assert count == len(pack) and got == pack, name
        assert counts == FP.counts(wi, hv, pack), name
        assert counts[4] - counts[5] == counts[0]
    assert counts[:4] == [0, 0, 0, 0]  # two handles with equal content: no bucket examined, no item gathered
    assert (_content(torch, want, max(len(wi), 1)), _content(torch, have, max(len(hi), 1))) == before
    for t in (want, have, empty, twin):
        t.close()


def test_what_the_id_cases_hold(stl, torch_cuda):
    """Neither kind of hash-keyed shortcut passes: a node of want whose hash have
    holds at another ID comes; a node at an ID have holds with another hash comes."""
    torch = torch_cuda
    wi, hi = FP.pair("hash_at_other_id")
    want, have = _tree(stl, torch, wi), _tree(stl, torch, hi)
    got, count, _ = _pack(stl, torch, want, have, 16).read()
    assert count == 7 and sorted(d for d, _ in got) == list(range(7))
    assert got[max(got)][0] in NM.hashes_of(NM.nodes_closed(hi))
    want.close(), have.close()
    wi, hi = FP.pair("same_id_other_hash")
    want, have = _tree(stl, torch, wi), _tree(stl, torch, hi)
    assert _pack(stl, torch, want, have, 64).read()[1] == 64
    want.close(), have.close()
    wi, hi = FP.pair("same_id_third_key")
    want, have = _tree(stl, torch, wi), _tree(stl, torch, hi)
    got, count, counts = _pack(stl, torch, want, have, 64).read()
    assert count == 31 and sorted(d for d, _ in got) == list(range(31)) and counts[5] == 33
    want.close(), have.close()


# ---- 2. have NULL: every inner node, as stl_shamap_nodes_device over the export gives them ----
@pytest.mark.parametrize("items", [0, 1, 2, 17, 300, 131073])
def test_against_none_equals_the_nodes_call_over_the_export(stl, torch_cuda, items):
    torch = torch_cuda
    keys = SM.case_keys(f"random{items}", 30 + items) if items else np.zeros((0, 32), np.uint8)
    leaves = np.random.default_rng(31).integers(0, 256, keys.shape, dtype=np.uint8)
    want = stl.ShamapTree(items + 3)
    if items:
        want.apply_device(_dev(torch, keys), _dev(torch, leaves))
    room = 2 * items + 8  # random keys: far fewer inner nodes than keys
    g = _pack(stl, torch, want, None, room)
    _, count, counts = g.read()
    k = torch.zeros((items + 3, 32), dtype=torch.uint8, device="cuda")
    l = torch.zeros((items + 3, 32), dtype=torch.uint8, device="cuda")
    want.export_device(k, l)
    _, c4, ref = stl.shamap_nodes_device(k[:items].contiguous(), l[:items].contiguous(), max_nodes=room)
    torch.cuda.synchronize()
    assert count == int(ref.count.item()) <= room and (items == 0 or count == int(c4[2]))
    rows = ref.rows()
    rm = ref.meta[:rows].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert NM.same_nodes(g.arrays(), (rm & 0xFF, ref.ids[:rows].cpu().numpy(), ref.hash[:rows].cpu().numpy(),
                                      ref.body[:rows].cpu().numpy(), rm >> 16))
    assert counts[0] == counts[4] == count and counts[5] == 0 and counts[6:] == [items, 0]
    want.close()


# ---- 3. kept and suppressed nodes in one tile ----
def test_mixed_tiles(stl, torch_cuda):
    """40,000 keys of one bucket in both trees, 300 leaf hashes differ: more
    than 128 nodes a depth, kept and suppressed ones side by side."""
    torch = torch_cuda
    rng = np.random.default_rng(40)
    keys = rng.integers(0, 256, (40000, 32), dtype=np.uint8)
    keys[:, 0], keys[:, 1] = 0xC3, 0x5A
    keys = np.unique(keys, axis=0)
    leaves = rng.integers(0, 256, keys.shape, dtype=np.uint8)
    other = leaves.copy()
    changed = rng.permutation(len(keys))[:300]
    other[changed] = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    hi = {k.tobytes(): v.tobytes() for k, v in zip(keys, leaves)}
    wi = {k.tobytes(): v.tobytes() for k, v in zip(keys, other)}
    want, have = _tree(stl, torch, wi), _tree(stl, torch, hi)
    wn, hn = NM.nodes_closed(wi), NM.nodes_closed(hi)
    pack = FP.pack_by_difference(wi, hi, wn, hn)
    per_depth = np.bincount([d for d, _ in wn], minlength=64)
    assert per_depth.max() > 128 and 0 < len(pack) < len(wn)
    got, count, counts = _pack(stl, torch, want, have, len(pack) + 3).read()
    assert count == len(pack) and got == pack
    assert counts[4] - counts[5] == counts[0] and counts[1:4] == [1, len(wi), len(hi)]
    assert counts[4] == len(wn) and counts[6:] == [len(wi), len(hi)]
    want.close(), have.close()


# ---- 4. after a fork ----
def test_after_a_fork_and_a_chain_of_three(stl, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(50)
    keys = SM.case_keys("random65536", 51)
    content = [{k.tobytes(): v.tobytes() for k, v in zip(keys, keys[:, ::-1])}]
    trees = [_tree(stl, torch, content[0], 70000)] + [stl.ShamapTree(70000) for _ in range(3)]
    e_first = None
    for step in range(3):
        batch = TM._mixed_batch(rng, content[-1], 256)
        dev = [None if a is None else _dev(torch, a) for a in batch]
        if step == 0:
            _, _, e_first = trees[0].fork_nodes_device(trees[1], *dev, max_nodes=40000)
        else:
            trees[step].fork_device(trees[step + 1], *dev)
        content.append(_applied(content[-1], *batch))
    torch.cuda.synchronize()
    nodes = {i: NM.nodes_closed(content[i]) for i in (0, 1, 3)}
    # the fork's own batch: the pack is the model's, a subset of E, and holds every node whose hash have lacks
    pack = FP.pack_by_difference(content[1], content[0], nodes[1], nodes[0])
    got, count, counts = _pack(stl, torch, trees[1], trees[0], len(pack) + 8).read()
    assert count == len(pack) and got == pack and counts == FP.counts(content[1], content[0], pack, nodes[1])
    e = NM.rows_as_dict(e_first.rows(), e_first.hash.cpu().numpy(), e_first.body.cpu().numpy(),
                        e_first.ids.cpu().numpy(), e_first.meta.cpu().numpy())
    assert all(e.get(k) == v for k, v in got.items()) and len(got) <= len(e)
    old_hashes = NM.hashes_of(nodes[0])
    assert all(k in got for k, v in nodes[1].items() if v[0] not in old_hashes)
    # three ledgers apart, both ways round
    for w, h in ((3, 0), (0, 3)):
        pack = FP.pack_by_difference(content[w], content[h], nodes[w], nodes[h])
        got, count, counts = _pack(stl, torch, trees[w], trees[h], len(pack) + 8).read()
        assert count == len(pack) and got == pack and counts[4] - counts[5] == counts[0]
    for t in trees:
        t.close()


# ---- 5. capacities ----
def test_capacities(stl, torch_cuda):
    torch = torch_cuda
    wi, hi = FP.pair("mixed300")
    a8 = dict(list(wi.items())[:8])
    b13 = {**dict(list(hi.items())[:10]), **dict(list(wi.items())[5:8])}
    for x, xc, y, yc in ((a8, 8, b13, 13), (b13, 13, a8, 8)):  # a full tree of 8 against a full tree of 13
        want, have = _tree(stl, torch, x, xc), _tree(stl, torch, y, yc)
        pack = FP.pack_by_difference(x, y)
        got, count, counts = _pack(stl, torch, want, have, _room(x)).read()
        assert count == len(pack) and got == pack and counts == FP.counts(x, y, pack)
        want.close(), have.close()
    # a stated bound above the count: deletes leave the host's bound loose
    want, have = _tree(stl, torch, wi, 1000), _tree(stl, torch, hi, 400)
    gone = list(wi)[:100]
    k = np.frombuffer(b"".join(gone), np.uint8).reshape(-1, 32)
    want.apply_device(_dev(torch, k), None, torch.ones(100, dtype=torch.uint8, device="cuda"))
    left = {key: v for key, v in wi.items() if key not in set(gone)}
    pack = FP.pack_by_difference(left, hi)
    got, count, counts = _pack(stl, torch, want, have, _room(wi)).read()
    assert count == len(pack) and got == pack and counts == FP.counts(left, hi, pack)
    want.close(), have.close()


# ---- 6. overflow, optional outputs, host forms ----
def test_overflow_optional_outputs_and_host_forms(stl, torch_cuda):
    torch = torch_cuda
    wi, hi = FP.pair("cluster_bucket")
    want, have = _tree(stl, torch, wi), _tree(stl, torch, hi)
    pack = FP.pack_by_difference(wi, hi)
    model_counts = FP.counts(wi, hi, pack)
    for room in (0, len(pack) - 1):
        got, count, counts = _pack(stl, torch, want, have, room).read()  # read(): no store passed `room` rows
        assert count == len(pack) and counts == model_counts
        assert len(got) == room and all(pack[k] == v for k, v in got.items())
    g = _pack(stl, torch, want, have, len(pack), ids=False, meta=False, counts=False)
    _, count, counts = g.read()
    assert count == len(pack) and counts is None
    assert sorted(h.tobytes() for h in g.hash[1:count + 1].cpu().numpy()) == sorted(v[0] for v in pack.values())
    by_hash = {v[0]: v[1] for v in pack.values()}
    assert all(by_hash[h.tobytes()] == b.tobytes() for h, b in zip(g.hash[1:count + 1].cpu().numpy(),
                                                                    g.body[1:count + 1].cpu().numpy()))
    # the host forms against the model (and so against the device forms)
    for hv_tree, hv in ((have, hi), (None, None)):
        p = FP.pack_by_difference(wi, hv)
        nodes, counts = want.fetch_pack(hv_tree, max_nodes=len(p) + 2)
        assert nodes.count == len(p) and counts == FP.counts(wi, hv, p)
        assert NM.rows_as_dict(nodes.rows(), nodes.hash, nodes.body, nodes.ids, nodes.meta) == p
    nodes, counts = want.fetch_pack(have, max_nodes=5, ids=False, meta=False)
    assert nodes.count == len(pack) and nodes.rows() == 5 and counts == model_counts
    assert all(h.tobytes() in by_hash for h in nodes.hash[:5])
    nodes, counts = want.fetch_pack(have, max_nodes=0)
    assert nodes.count == len(pack) and counts == model_counts
    want.close(), have.close()


# ---- 7. read-only, side by side ----
def test_two_packs_on_two_streams_leave_the_trees_alone(stl, torch_cuda):
    torch = torch_cuda
    wi, hi = FP.pair("mixed300")
    want, have = _tree(stl, torch, wi, 400), _tree(stl, torch, hi, 350)
    probes = _dev(torch, np.frombuffer(b"".join(list(wi)[:200] + list(hi)[:200]), np.uint8).reshape(-1, 32))

    def state():
        out = []
        for t in (want, have):
            w, l, p = t.lookup_device(probes, leaf_hashes=True, positions=True)
            out += [w, l, p]
        d = want.compare_device(have, 1000)
        rows = d.rows()  # waits
        out = [x.cpu().numpy().tobytes() for x in out + [d.key[:rows], d.kind[:rows], d.leaf_a[:rows],
                                                         d.leaf_b[:rows], d.counts]]
        return out + [_content(torch, want, 400), _content(torch, have, 350)]

    before = state()
    pack = FP.pack_by_difference(wi, hi)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a = _pack(stl, torch, want, have, len(pack), stream=s1)  # enqueued back to back, no wait between them
    b = _pack(stl, torch, want, have, len(pack), stream=s2)
    for g in (a, b):
        got, count, counts = g.read()
        assert count == len(pack) and got == pack and counts == FP.counts(wi, hi, pack)
    assert state() == before
    want.close(), have.close()


# ---- 8. the failure contract ----
@pytest.mark.parametrize("form", ["device", "device_none", "host"])
def test_fault_injection(stl, torch_cuda, form):
    """Every HIP call of one fetch pack failed in turn (at the API boundary: no
    device fault): the call returns < 0, the count words keep their guard value,
    both trees are unchanged, and the same call afterwards gives the model's pack."""
    from stellard_amd import _native as N
    torch = torch_cuda
    wi, hi = FP.pair("cluster_prefix10")
    want, have = _tree(stl, torch, wi), _tree(stl, torch, hi)
    hv_tree, hv = (None, None) if form == "device_none" else (have, hi)
    pack = FP.pack_by_difference(wi, hv)
    before = _content(torch, want, len(wi)), _content(torch, have, len(hi))
    stream = torch.cuda.Stream()  # a fresh context: the first call also allocates
    failed, kk = 0, 0
    try:
        while True:
            assert kk < 400, "the countdown never ran out"
            g = Guarded(stl, torch, len(pack))
            host_counts = None
            torch.cuda.synchronize()
            stl.debug_fault_after(kk)
            kk += 1
            try:
                if form == "host":
                    nodes, host_counts = want.fetch_pack(hv_tree, max_nodes=len(pack))
                else:
                    want.fetch_pack_device(hv_tree, nodes=g.nodes, counts=g.counts[8:16], stream=stream)
                    torch.cuda.synchronize()
            except N.StlError as e:
                assert e.rc < 0
                failed += 1
                stl.debug_fault_after(-1)
                torch.cuda.synchronize()
                assert g.untouched(), kk
                assert (_content(torch, want, len(wi)), _content(torch, have, len(hi))) == before, kk
                continue
            stl.debug_fault_after(-1)
            if form == "host":
                assert nodes.count == len(pack) and host_counts == FP.counts(wi, hv, pack)
                assert NM.rows_as_dict(nodes.rows(), nodes.hash, nodes.body, nodes.ids, nodes.meta) == pack
            else:
                got, count, counts = g.read()
                assert count == len(pack) and got == pack and counts == FP.counts(wi, hv, pack)
            break  # no call left to fail
    finally:
        stl.debug_fault_after(-1)
    torch.cuda.synchronize()
    assert failed == kk - 1
    # the memset, the buckets, two scans, gather and neighbours per side, 60 level launches per side, four top
    # launches and the finish
    least = {"device": 1 + 1 + 4 + 4 + 120 + 5, "device_none": 1 + 1 + 2 + 2 + 60 + 5, "host": 1 + 1 + 4 + 4 + 120 + 5}
    assert failed >= least[form], (form, failed)
    assert (_content(torch, want, len(wi)), _content(torch, have, len(hi))) == before
    want.close(), have.close()


def test_handles_that_are_not_live(stl, torch_cuda):
    from stellard_amd import _native as N
    torch = torch_cuda
    wi, _ = FP.pair("one_key")
    want = _tree(stl, torch, wi)
    dead = stl.ShamapTree(16)
    h = dead.handle.value
    dead.close()
    g = Guarded(stl, torch, 4)
    out = g.nodes.struct()
    import ctypes
    lib = N.load()
    for w, hv in ((h, None), (want.handle.value, h), (h, want.handle.value), (h, h)):
        assert lib.stl_shamap_tree_fetch_pack_device(w, hv, ctypes.byref(out), None, None) == N.STL_EINVAL
        assert lib.stl_shamap_tree_fetch_pack(w, hv, ctypes.byref(out), None) == N.STL_EINVAL
    torch.cuda.synchronize()
    assert g.untouched()
    want.close()


# ---- 9. phase timing ----
def test_phase_timing_counts_the_call(stl, torch_cuda):
    torch = torch_cuda
    wi, hi = FP.pair("mixed300")
    want, have = _tree(stl, torch, wi), _tree(stl, torch, hi)
    torch.cuda.synchronize()
    stl.reset_stats()
    stl.set_phase_timing(True)
    try:
        _pack(stl, torch, want, have, 8).read()
        st = stl.get_stats()
    finally:
        stl.set_phase_timing(False)
    ph = list(st["phase_ns"].values())
    assert st["phase_chunks"] == 1 and all(v > 0 for v in ph[:3])
    want.close(), have.close()


# ---- 10. the fixture ----
def test_golden_packs(stl, torch_cuda):
    torch = torch_cuda
    with open(FP.GOLDEN) as f:
        doc = json.load(f)
    for p in doc["packs"]:
        wi, hi = FP.pair(p["pair"])
        want = _tree(stl, torch, wi)
        have = _tree(stl, torch, hi) if p["against"] == "have" else None
        got, count, counts = _pack(stl, torch, want, have, len(p["pack"]) + 1).read()
        assert want.root_device()[0].cpu().numpy().tobytes().hex() == p["want_root"]
        assert sorted((d, nid.hex(), v[0].hex(), v[2]) for (d, nid), v in got.items()) == [
            (n["depth"], n["id"], n["hash"], n["leaf_mask"]) for n in p["pack"]]
        assert counts == p["counts"] and count == len(p["pack"])
        want.close()
        if have is not None:
            have.close()
