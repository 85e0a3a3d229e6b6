"""The fetch pack of one SHAMap against another (stl_shamap_tree_fetch_pack*) in
Python: the model the host emulation and the GPU calls are tested against, on
top of tests/shamap_py.py, tests/shamap_nodes_py.py and tests/shamap_lookup_py.py.

For a tree `want` and a tree `have` (or None) the pack is every inner node of
want, at (depth, masked key), for which have holds no inner node at the same ID
with the same hash.  Two independent statements:

  * pack_by_difference: the set difference over shamap_nodes_py.nodes_closed;
  * pack_by_walk: SHAMap::getFetchPack's stack walk over shamap_py's insertion
    tree -- a node is emitted and an inner child pushed only when
    not has_inner_node(have, child ID, child hash), where has_inner_node descends
    have by the ID, nibble by nibble, and compares the hash it finds there.  The
    walk also gives the pack's leaves (not has_leaf_node(have, key, hash)).

counts() gives the eight counts of the call by the bucket rule; pairs() the
seeded pairs of maps the tests share; the rest binds the host emulation."""
import ctypes
import os

import numpy as np

from tests import shamap_lookup_py as LM
from tests import shamap_nodes_py as NM
from tests import shamap_py as SM
from tests import shamap_tree_py as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FETCH_SO = os.path.join(ROOT, "tests", "native", "libhostemu_shamap_fetch.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "shamap_fetch.json")


# ---- 1. the set difference ----
def pack_by_difference(want, have, want_nodes=None, have_nodes=None):
    """want, have: {key: leaf hash} (have may be None) -> {(depth, id): (hash, body, leaf mask)}."""
    wn = NM.nodes_closed(want) if want_nodes is None else want_nodes
    hn = (NM.nodes_closed(have) if have else {}) if have_nodes is None else have_nodes
    return {k: v for k, v in wn.items() if k not in hn or hn[k][0] != v[0]}


# ---- 2. the reference's walk ----
class _Hashed:
    """An insertion tree with every inner node's hash."""

    def __init__(self, items):
        self.root = SM._Inner()
        for k, h in items.items():
            assert SM.insert(self.root, bytes(k), bytes(h))
        self.empty = not items
        self.hash = {}
        stack = [(self.root, False)]
        while stack:
            n, seen = stack.pop()
            if not seen:
                stack.append((n, True))
                stack.extend((c, False) for c in n.child if isinstance(c, SM._Inner))
                continue
            self.hash[id(n)] = SM.inner_hash([self.child_hash(n, b) for b in range(16)])

    def child_hash(self, n, b):
        c = n.child[b]
        if c is None:
            return SM.ZERO
        return c.hash if isinstance(c, SM._Leaf) else self.hash[id(c)]

    def root_hash(self):
        return SM.ZERO if self.empty else self.hash[id(self.root)]


def has_inner_node(tree, depth, node_id, node_hash):
    """SHAMap::hasInnerNode: descend by the ID's nibbles to its depth."""
    node, d = tree.root, 0
    while isinstance(node, SM._Inner) and d < depth:
        nxt = node.child[SM.nibble(node_id, d)]
        if nxt is None:
            return False
        node, d = nxt, d + 1
    return isinstance(node, SM._Inner) and tree.hash[id(node)] == node_hash


def has_leaf_node(tree, key, leaf_hash):
    """SHAMap::hasLeafNode: on the way down by the key, a child hash that matches."""
    node, d = tree.root, 0
    while True:
        b = SM.nibble(key, d)
        if node.child[b] is None:
            return False
        if tree.child_hash(node, b) == leaf_hash:
            return True
        node, d = node.child[b], d + 1
        if not isinstance(node, SM._Inner):
            return False


def pack_by_walk(want, have):
    """-> (the inner nodes as pack_by_difference gives them, the leaves {key: leaf hash})."""
    w = _Hashed(want)
    h = _Hashed(have) if have is not None else None
    nodes, leaves = {}, {}
    if w.root_hash() == SM.ZERO:
        return nodes, leaves
    if h is not None and w.root_hash() == h.root_hash():
        return nodes, leaves
    stack = [(w.root, 0, bytes(32))]
    while stack:
        node, d, nid = stack.pop()
        slots = [w.child_hash(node, b) for b in range(16)]
        mask = sum(1 << b for b in range(16) if isinstance(node.child[b], SM._Leaf))
        assert (d, nid) not in nodes
        nodes[(d, nid)] = (w.hash[id(node)], b"".join(slots), mask)
        for b in range(16):
            c = node.child[b]
            if c is None:
                continue
            if isinstance(c, SM._Inner):
                cid = bytearray(nid)
                cid[d >> 1] |= b if d & 1 else b << 4
                cid = bytes(cid)
                if h is None or not has_inner_node(h, d + 1, cid, slots[b]):
                    stack.append((c, d + 1, cid))
            elif h is None or not has_leaf_node(h, c.key, slots[b]):
                leaves[c.key] = c.hash
    return nodes, leaves


# ---- the counts ----
def counts(want, have, pack=None, want_nodes=None):
    """The call's eight counts: the bucket rule gathers the differing buckets
    where want holds two keys or more (and of have where both do); a candidate
    is an inner node of want in such a bucket or above the buckets."""
    hv = have or {}
    bw, bh = LM.by_bucket(want), LM.by_bucket(hv)
    examined = gathered_w = gathered_h = 0
    taken = set()
    for b in sorted(set(bw) | set(bh)):
        sw, sh = bw.get(b, {}), bh.get(b, {})
        if not LM.bucket_differs(sw, sh, b):
            continue
        examined += 1
        if len(sw) >= 2:
            gathered_w += len(sw)
            taken.add(b)
            if len(sh) >= 2:
                gathered_h += len(sh)
    wn = NM.nodes_closed(want) if want_nodes is None else want_nodes
    cand = sum(1 for (d, nid) in wn if d < 4 or ((nid[0] << 8) | nid[1]) in taken)
    pack = pack_by_difference(want, have, wn) if pack is None else pack
    return [len(pack), examined, gathered_w, gathered_h, cand, cand - len(pack), len(want), len(hv)]


# ---- the shared pairs ----
def _rand(rng, n=1):
    return [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]


def _under(prefix_hex, rng, n):
    """n random keys under a nibble prefix."""
    out = []
    for k in _rand(rng, n):
        hx = prefix_hex + k.hex()[len(prefix_hex):]
        out.append(bytes.fromhex(hx))
    return out


def _last_nibble_pair(rng):
    k = bytearray(_rand(rng)[0])
    a, b = bytes(k[:31] + bytes([(k[31] & 0xF0) | 0x3])), bytes(k[:31] + bytes([(k[31] & 0xF0) | 0xC]))
    return a, b


PAIRS = ["both_empty", "want_empty", "have_empty", "same", "one_key", "one_key_other_leaf", "hash_at_other_id",
         "same_id_other_hash", "same_id_third_key", "buckets_ends", "bucket_want_only", "bucket_have_only",
         "bucket_2_1", "bucket_1_2", "below_depth_10", "mixed300", "cluster_bucket", "cluster_prefix10"]


def pair(name):
    """A seeded pair ({key: leaf}, {key: leaf}) by name: want, have."""
    rng = np.random.default_rng(900 + PAIRS.index(name))
    base = {k: v for k, v in zip(_rand(rng, 40), _rand(rng, 40))}
    if name == "both_empty":
        return {}, {}
    if name == "want_empty":
        return {}, base
    if name == "have_empty":
        return base, {}
    if name == "same":
        return base, dict(base)
    if name == "one_key":
        k = _rand(rng)[0]
        return {k: k}, {}
    if name == "one_key_other_leaf":
        k, v = _rand(rng, 2)
        return {k: k}, {k: v}
    if name == "hash_at_other_id":
        # three leaf hashes under aabbcc in want and under 112233 in have, parting at nibble 6 on the
        # same branches: the node at depth 6 has the same hash in both trees, at different IDs, and
        # all 7 nodes of want belong in the pack
        want, have = {}, {}
        for i, (t, v) in enumerate(zip(_rand(rng, 3), _rand(rng, 3))):
            tail = "%x" % (3 + 5 * i) + t.hex()[7:]
            want[bytes.fromhex("aabbcc" + tail)] = v
            have[bytes.fromhex("112233" + tail)] = v
        return want, have
    if name == "same_id_other_hash":
        a, b = _last_nibble_pair(rng)
        v = _rand(rng, 3)
        return {a: v[0], b: v[1]}, {a: v[0], b: v[2]}
    if name == "same_id_third_key":
        a, b = _last_nibble_pair(rng)
        v = _rand(rng, 3)
        third = bytearray(a)
        third[15] ^= 0x80  # shares 30 nibbles, parts at nibble 30
        return {a: v[0], b: v[1]}, {a: v[0], b: v[1], bytes(third): v[2]}
    if name == "buckets_ends":
        want = dict(base)
        for k, v in zip(_under("0000", rng, 3) + _under("ffff", rng, 3) + _under("7777", rng, 3), _rand(rng, 9)):
            want[k] = v
        have = dict(want)
        for p in ("0000", "ffff"):
            k = next(k for k in sorted(have) if k.hex().startswith(p))
            have[k] = _rand(rng)[0]
        return want, have
    if name == "bucket_want_only":
        want = dict(base)
        for k, v in zip(_under("4242", rng, 4), _rand(rng, 4)):
            want[k] = v
        return want, dict(base)
    if name == "bucket_have_only":
        have = dict(base)
        for k, v in zip(_under("4242", rng, 4), _rand(rng, 4)):
            have[k] = v
        return dict(base), have
    if name in ("bucket_2_1", "bucket_1_2"):
        ks, vs = _under("5151", rng, 2), _rand(rng, 2)
        two = {**base, ks[0]: vs[0], ks[1]: vs[1]}
        one = {**base, ks[0]: vs[0]}
        return (one, two) if name == "bucket_2_1" else (two, one)
    if name == "below_depth_10":
        ks = _under("6a6a6a6a6a", rng, 5) + _under("6a6a", rng, 3)
        want = {**base, **{k: k for k in ks}}
        have = dict(want)
        have[ks[0]] = _rand(rng)[0]
        return want, have
    if name == "mixed300":
        big = {k: v for k, v in zip(_rand(rng, 300), _rand(rng, 300))}
        have, want = LM.derive(big, rng, 20, 30, 25)
        return want, have
    if name == "cluster_bucket":
        ks = _under("9c9c", rng, 200)
        big = {k: v for k, v in zip(ks, _rand(rng, 200))}
        have, want = LM.derive(big, rng, 5, 0, 12)
        for k in _under("9c9c", rng, 6):
            want[k] = k
        return want, have
    if name == "cluster_prefix10":
        ks = _under("0123456789", rng, 150) + _rand(rng, 30)
        big = {k: v for k, v in zip(ks, _rand(rng, 180))}
        have, want = LM.derive(big, rng, 8, 4, 10)
        return want, have
    raise KeyError(name)


def generated_pairs(n, seed):
    """n small random pairs with sets, replaces, deletes and near-collisions."""
    rng = np.random.default_rng(seed)
    for i in range(n):
        kind = i % 3
        m = int(rng.integers(1, 24))
        if kind == 0:
            ks = _rand(rng, m)
        elif kind == 1:
            ks = _under("3d3d", rng, m)
        else:
            ks = _under("3d3d3d3d3d", rng, m)
        have = {k: v for k, v in zip(ks, _rand(rng, m))}
        want = dict(have)
        for k in list(want):
            r = rng.random()
            if r < 0.15:
                del want[k]
            elif r < 0.3:
                want[k] = _rand(rng)[0]
            elif r < 0.4:
                near = bytearray(k)
                near[int(rng.integers(2, 32))] ^= 1 << int(rng.integers(0, 8))
                want[bytes(near)] = _rand(rng)[0]
        yield want, have


# ---- the fixture ----
GOLDEN_PAIRS = ["one_key", "hash_at_other_id", "same_id_third_key", "bucket_2_1", "below_depth_10"]


def golden_document():
    """What tests/golden/shamap_fetch.json holds: a few pairs and their packs, hashes and IDs."""
    out = []
    for name in GOLDEN_PAIRS:
        want, have = pair(name)
        for label, hv in (("have", have), ("none", None)):
            p = pack_by_difference(want, hv)
            out.append({"pair": name, "against": label, "want_root": SM.root_recursive(want)[0].hex(),
                        "have_root": SM.root_recursive(hv or {})[0].hex(), "counts": counts(want, hv, p),
                        "pack": [{"depth": d, "id": nid.hex(), "hash": v[0].hex(), "leaf_mask": v[2]}
                                 for (d, nid), v in sorted(p.items())]})
    return {"packs": out}


# ---- the host emulation ----
def load_fetch_emu():
    from stellard_amd import build
    build.build_hostemu_shamap_fetch()
    lib = ctypes.CDLL(FETCH_SO)
    V, U, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    for name, res, args in (
            ("hostemu_fetch_want_rows", U, [I, U]),
            ("hostemu_fetch_have_rows", U, [I, U, U]),
            ("hostemu_fetch_top_inner", I, [U, I]),
            ("hostemu_fetch_top_keeps", I, [V, U, V, I]),
            ("hostemu_fetch_top_value_agrees", I, [V, V, I]),
            ("hostemu_fetch_have_holds", I, [V, V, V, U, V, U, V]),
            ("hostemu_fetch_pack", I, [V, V, V, V, U, V, V, V, V, U, I, U, V, V, V, V, V, V])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def emu_pack(emu, want, have, max_nodes=None, ids=True, meta=True):
    """The staged call on generations of exactly their trees' sizes -> (EmuOut, counts)."""
    gw = LM.EmuGen(want)
    gh = LM.EmuGen(have) if have is not None else None
    if max_nodes is None:
        max_nodes = 63 * max(len(want) - 1, 0) + 1
    out = NM.EmuOut(max_nodes, ids, meta)
    cnt = np.full(8, 0xA5A5A5A5, np.uint32)
    p = LM._p
    hargs = (p(gh.key), p(gh.leaf), p(gh.bcnt), p(gh.bh), gh.m, 1) if gh is not None else (None, None, None, None, 0, 0)
    rc = emu.hostemu_fetch_pack(p(gw.key), p(gw.leaf), p(gw.bcnt), p(gw.bh), gw.m, *hargs, *out.args(), p(cnt))
    assert rc == 0, rc
    return out, [int(x) for x in cnt]
