"""A SHAMap's nodes by node ID and its paths by key
(stl_shamap_tree_get_nodes*: SHAMap::getNodeFat and SHAMap::getPath) in Python:
the model the host emulation and the GPU calls are tested against, on top of
tests/shamap_py.py and tests/shamap_nodes_py.py.

A request is (id, depth, mode); its answer is

    (status, [(depth, masked key) of every row, in order], leaf key or None)

stated twice:

  * answer_by_walk: over shamap_py's insertion tree, what the reference's loops
    do -- getNodeFat descends by the ID's nibbles while the node is inner and
    shallower than wanted, compares the ID it arrived at, emits the node and
    then follows the chain `do .. while (count == 1 && node->isInner())`,
    emitting inner children only (fatLeaves is false); getPath pushes every
    inner node on the way down the key;
  * answer_closed: the closed form over the sorted keys -- ranges of keys under
    a nibble prefix, nothing else.

answer() adds what the rows hold (hash, body, leaf mask from
shamap_nodes_py.nodes_closed) and the call's eight counts.  Also the named
cases, the generated batches, the golden document and the binding of the host
emulation."""
import bisect
import ctypes
import os

import numpy as np

from tests import shamap_lookup_py as LM
from tests import shamap_nodes_py as NM
from tests import shamap_py as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GET_SO = os.path.join(ROOT, "tests", "native", "libhostemu_shamap_get.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "shamap_get.json")

NODE, FAT, PATH = 0, 1, 2
ABSENT, INNER, LEAF, EMPTY_ROOT, INVALID, OTHER_LEAF = 0, 1, 2, 3, 4, 5
MAX_ROWS = 80
MAX_REQUESTS = 1 << 24


# ---- 1. the reference's walks ----
def _tree(items):
    root = SM._Inner()
    for k, h in items.items():
        assert SM.insert(root, bytes(k), bytes(h))
    return root


def _child_id(nid, d, b):
    out = bytearray(nid)
    out[d >> 1] |= b if d & 1 else b << 4
    return bytes(out)


def answer_by_walk(items, nid, depth, mode, root=None):
    root = _tree(items) if root is None else root
    nid = bytes(nid)
    if mode not in (NODE, FAT, PATH):
        return INVALID, [], None
    if mode == PATH:
        if not items:
            return ABSENT, [], None  # the contract: an empty tree has no row
        node, at, d, rows = root, bytes(32), 0, []
        while isinstance(node, SM._Inner):
            rows.append((d, at))
            b = SM.nibble(nid, d)
            if node.child[b] is None:
                return ABSENT, rows, None
            node, at, d = node.child[b], _child_id(at, d, b), d + 1
        return (LEAF if node.key == nid else OTHER_LEAF), rows, node.key
    if depth > 63:  # SHAMapNodeID::isValid
        return INVALID, [], None
    node, at, d = root, bytes(32), 0
    while node is not None and isinstance(node, SM._Inner) and d < depth:
        b = SM.nibble(nid, d)
        node, at, d = node.child[b], _child_id(at, d, b), d + 1
    if node is None or (d, at) != (depth, nid):
        return ABSENT, [], None
    if isinstance(node, SM._Leaf):
        return LEAF, [], node.key
    if all(c is None for c in node.child):
        return EMPTY_ROOT, [], None
    rows = [(d, at)]
    if mode == NODE:
        return INNER, rows, None
    while True:
        count, nxt = 0, None
        for b in range(16):
            c = node.child[b]
            if c is None:
                continue
            count += 1
            nxt = (c, _child_id(at, d, b))
            if isinstance(c, SM._Inner):
                rows.append((d + 1, nxt[1]))
        if count != 1 or not isinstance(nxt[0], SM._Inner):
            return INNER, rows, None
        node, at, d = nxt[0], nxt[1], d + 1


# ---- 2. the closed form ----
class Closed:
    """The sorted keys of a tree as hex strings: a nibble prefix is a string prefix."""

    def __init__(self, items):
        self.keys = sorted(bytes(k) for k in items)
        self.hex = [k.hex() for k in self.keys]

    def range(self, prefix):
        return bisect.bisect_left(self.hex, prefix), bisect.bisect_left(self.hex, prefix + "g")

    def answer(self, nid, depth, mode):
        nid = bytes(nid)
        hx = nid.hex()
        if mode not in (NODE, FAT, PATH):
            return INVALID, [], None
        if mode == PATH:
            if not self.keys:
                return ABSENT, [], None
            D = 1
            while D < 64 and self.range(hx[:D])[1] - self.range(hx[:D])[0] >= 2:
                D += 1
            rows = [(d, NM.masked(nid, d)) for d in range(D)]
            lo, hi = self.range(hx[:D])
            if hi == lo:
                return ABSENT, rows, None
            assert hi - lo == 1
            return (LEAF if self.keys[lo] == nid else OTHER_LEAF), rows, self.keys[lo]
        if depth > 63:
            return INVALID, [], None
        if NM.masked(nid, depth) != nid:
            return ABSENT, [], None
        lo, hi = self.range(hx[:depth])
        c = hi - lo
        if c >= 2 or (depth == 0 and c == 1):
            if mode == NODE or c == 1:
                return INNER, [(depth, nid)], None
            L = SM.common_prefix(self.keys[lo], self.keys[hi - 1])
            first = self.keys[lo]
            rows = [(d, NM.masked(first, d)) for d in range(depth, L + 1)]
            for b in range(16):
                p = first.hex()[:L] + "%x" % b
                plo, phi = self.range(p)
                if phi - plo >= 2:
                    rows.append((L + 1, NM.masked(self.keys[plo], L + 1)))
            return INNER, rows, None
        if depth == 0:
            return EMPTY_ROOT, [], None
        if c == 1:
            plo, phi = self.range(hx[:depth - 1])
            if depth == 1 or phi - plo >= 2:
                return LEAF, [], self.keys[lo]
        return ABSENT, [], None


def answer_closed(items, nid, depth, mode):
    return Closed(items).answer(nid, depth, mode)


# ---- the whole call ----
class Answer:
    """What one call writes for a batch of requests against `items`."""

    def __init__(self, items, requests, max_nodes=None, nodes=None):
        cl = Closed(items)
        nodes = NM.nodes_closed(items) if nodes is None else nodes
        self.status, self.first, self.rows, self.leaf_key, self.leaf_hash, self.row_ids = [], [], [], [], [], []
        for nid, depth, mode in requests:
            st, rows, leaf = cl.answer(nid, depth, mode)
            assert len(rows) <= MAX_ROWS
            self.status.append(st)
            self.first.append(len(self.row_ids))
            self.rows.append(len(rows))
            self.leaf_key.append(leaf if leaf is not None else bytes(32))
            self.leaf_hash.append(bytes(items[leaf]) if leaf is not None else bytes(32))
            self.row_ids.extend(rows)
        self.total = len(self.row_ids)
        self.max_nodes = self.total if max_nodes is None else max_nodes
        self.node = [(d, nid) + nodes[(d, nid)] for d, nid in self.row_ids]  # (depth, id, hash, body, leaf mask)
        stored = self.row_ids[:self.max_nodes]
        buckets = {(nid[0] << 8) | nid[1] for d, nid in stored if d >= 4}
        by_bucket = LM.by_bucket(items)
        self.counts = [self.total, sum(s == INNER for s in self.status),
                       sum(s in (LEAF, OTHER_LEAF) for s in self.status),
                       sum(s in (ABSENT, EMPTY_ROOT, INVALID) for s in self.status), len(buckets),
                       sum(len(by_bucket[b]) for b in buckets), len(set(stored)), len(items)]


def request_arrays(requests):
    """-> (ids uint8[n, 32], depths uint8[n], modes uint8[n])."""
    n = len(requests)
    ids = np.frombuffer(b"".join(bytes(r[0]) for r in requests), np.uint8).reshape(n, 32).copy() if n else \
        np.zeros((0, 32), np.uint8)
    return ids, np.array([r[1] for r in requests], np.uint8), np.array([r[2] for r in requests], np.uint8)


def check_outputs(ans, status, first, rows, leaf_key, leaf_hash, hashes, body, ids, meta, count, counts=None):
    """A call's outputs (numpy; leaf arrays, ids and meta may be None) against the model."""
    n = len(ans.status)
    assert [int(x) for x in status[:n]] == ans.status
    assert [int(x) for x in first[:n]] == ans.first
    assert [int(x) for x in rows[:n]] == ans.rows
    if leaf_key is not None:
        assert [bytes(r) for r in np.asarray(leaf_key)[:n]] == ans.leaf_key
    if leaf_hash is not None:
        assert [bytes(r) for r in np.asarray(leaf_hash)[:n]] == ans.leaf_hash
    assert int(count) == ans.total
    for r in range(min(ans.total, ans.max_nodes)):
        d, nid, h, b, mask = ans.node[r]
        assert bytes(hashes[r]) == h, ("hash", r)
        assert bytes(body[r]) == b, ("body", r)
        if ids is not None:
            assert bytes(ids[r]) == nid, ("id", r)
        if meta is not None:
            assert int(meta[r]) & 0xFFFFFFFF == NM.meta_word(d, mask), ("meta", r)
    if counts is not None:
        assert [int(x) for x in counts] == ans.counts


# ---- the named cases ----
def _rand(rng, n=1):
    return [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]


def _under(prefix_hex, rng, n):
    return [bytes.fromhex(prefix_hex + k.hex()[len(prefix_hex):]) for k in _rand(rng, n)]


def _with_nibble(key, d, v):
    out = bytearray(key)
    out[d >> 1] = (out[d >> 1] & 0x0F) | (v << 4) if not d & 1 else (out[d >> 1] & 0xF0) | v
    return bytes(out)


def _items(keys, rng):
    return {k: v for k, v in zip(keys, _rand(rng, len(keys)))}


def _pair63(rng):
    k = _rand(rng)[0]
    return _with_nibble(k, 63, 3), _with_nibble(k, 63, 12)


CASES = ["empty", "one_key", "two_first_nibble", "pair63", "pair63_third", "seventeen_buckets", "seventeen_one_bucket",
         "thrice", "parent_child", "all_modes", "mode_null", "unknown_mode"]
ROOT_ID = bytes(32)


def case(name):
    """A seeded (items, requests, modes given) by name; modes given False: the call passes d_mode NULL."""
    rng = np.random.default_rng(2300 + CASES.index(name))
    M = NM.masked
    if name == "empty":
        k = _rand(rng)[0]
        return {}, [(ROOT_ID, 0, NODE), (ROOT_ID, 0, FAT), (M(k, 1), 1, FAT), (k, 0, PATH), (k, 0, FAT)], True
    if name == "one_key":
        k, o = _rand(rng, 2)
        o = _with_nibble(o, 0, SM.nibble(k, 0) ^ 5)            # another branch of the root
        near = _with_nibble(k, 40, SM.nibble(k, 40) ^ 1)       # the same branch: ends at the leaf k
        return _items([k], rng), [(ROOT_ID, 0, NODE), (ROOT_ID, 0, FAT), (M(k, 1), 1, NODE), (M(k, 1), 1, FAT),
                                  (M(k, 2), 2, FAT), (k, 0, PATH), (near, 9, PATH), (o, 0, PATH)], True
    if name == "two_first_nibble":
        a, b = _rand(rng, 2)
        a, b = _with_nibble(a, 0, 2), _with_nibble(b, 0, 11)
        return _items([a, b], rng), [(ROOT_ID, 0, FAT), (ROOT_ID, 0, NODE), (M(a, 1), 1, FAT), (M(b, 1), 1, NODE),
                                     (M(a, 2), 2, FAT), (_with_nibble(ROOT_ID, 0, 5), 1, FAT), (a, 0, PATH),
                                     (b, 0, PATH)], True
    if name in ("pair63", "pair63_third"):
        a, b = _pair63(rng)
        keys = [a, b]
        rq = [(ROOT_ID, 0, FAT), (M(a, 3), 3, NODE), (M(a, 4), 4, NODE), (M(a, 63), 63, NODE), (a, 0, PATH),
              (b, 0, PATH), (M(a, 1), 1, FAT), (M(a, 63), 63, FAT), (a, 64, FAT), (a, 255, NODE),
              (_with_nibble(a, 63, 7), 0, PATH), (M(a, 30), 31, FAT)]
        if name == "pair63_third":
            keys.append(_with_nibble(_rand(rng)[0], 0, SM.nibble(a, 0) ^ 9))
            rq.append((keys[2], 0, PATH))
        return _items(keys, rng), rq, True
    if name == "seventeen_buckets":
        # 16 two-key buckets under one depth-3 prefix, and a key elsewhere
        keys = []
        for c in range(16):
            keys += _under("7a3%x" % c, rng, 2)
        keys += _under("1", rng, 1)
        k = keys[0]
        return _items(keys, rng), [(M(k, 3), 3, FAT), (ROOT_ID, 0, FAT), (M(k, 4), 4, FAT), (M(k, 3), 3, NODE),
                                   (keys[5], 0, PATH)], True
    if name == "seventeen_one_bucket":
        keys = _under("c4d2", rng, 17)
        k = sorted(keys)[8]
        return _items(keys, rng), [(ROOT_ID, 0, FAT), (M(k, 4), 4, FAT), (M(k, 5), 5, FAT), (M(k, 4), 4, NODE),
                                   (k, 0, PATH), (M(k, 2), 2, NODE)], True
    if name in ("thrice", "parent_child", "all_modes", "mode_null", "unknown_mode"):
        keys = _under("5e5e1", rng, 6) + _under("5e5e", rng, 5) + _rand(rng, 20)
        items = _items(keys, rng)
        k = sorted(x for x in keys if x.hex().startswith("5e5e1"))[0]
        if name == "thrice":
            return items, [(M(k, 4), 4, FAT)] * 3 + [(ROOT_ID, 0, FAT)] * 3, True
        if name == "parent_child":
            return items, [(M(k, 4), 4, FAT), (M(k, 3), 3, FAT), (M(k, 5), 5, FAT), (M(k, 2), 2, FAT)], True
        if name == "all_modes":
            return items, [(M(k, 4), 4, NODE), (M(k, 4), 4, FAT), (k, 0, PATH), (ROOT_ID, 0, NODE),
                           (_rand(rng)[0], 77, PATH)], True
        if name == "mode_null":
            return items, [(M(k, 4), 4, FAT), (ROOT_ID, 0, FAT), (M(keys[-1], 1), 1, FAT), (M(k, 6), 6, FAT)], False
        return items, [(M(k, 4), 4, 3), (ROOT_ID, 0, 255), (ROOT_ID, 0, FAT), (k, 0, 7)], True
    raise KeyError(name)


# ---- generated batches ----
def requests_for(items, rng, n):
    """n requests against a tree: IDs of existing inner nodes at every depth and
    of leaves, their mutations, and paths of present and absent keys."""
    cl = Closed(items)
    keys = cl.keys or _rand(rng, 1)
    out = []
    for _ in range(n):
        i = int(rng.integers(0, len(keys)))
        k = keys[i]
        r = int(rng.integers(0, 12))
        # the depth of k's leaf: one past the longest prefix it shares with another key, a neighbour in key order
        others = [SM.common_prefix(k, keys[j]) for j in (i - 1, i + 1) if 0 <= j < len(keys)]
        leaf_depth = (max(others) if others else 0) + 1
        d = int(rng.integers(0, leaf_depth))  # an inner node on k's way
        mode = int(rng.integers(0, 2))
        if r < 4:
            out.append((NM.masked(k, d), d, mode))
        elif r == 4:
            out.append((NM.masked(k, leaf_depth), leaf_depth, mode))              # the leaf
        elif r == 5:
            out.append((k, d, mode))                                               # unmasked
        elif r == 6:
            out.append((NM.masked(_rand(rng)[0], max(d, 1)), max(d, 1), mode))     # a prefix with no key, mostly
        elif r == 7:
            e = min(leaf_depth + 1, 63)
            out.append((NM.masked(k, e), e, mode))                                 # one nibble past a leaf
        elif r == 8:
            out.append((NM.masked(k, d), 64 if rng.integers(0, 2) else 255, mode))
        elif r == 9:
            out.append((k, int(rng.integers(0, 256)), PATH))                       # present
        elif r == 10:
            dd = int(rng.integers(leaf_depth, 64)) if leaf_depth < 64 else 63
            out.append((_with_nibble(k, dd, SM.nibble(k, dd) ^ 1), 0, PATH))       # absent next to a leaf
        else:
            dd = int(rng.integers(0, leaf_depth))
            out.append((_with_nibble(k, dd, int(rng.integers(0, 16))), 0, PATH))   # often into an empty branch
    return out


def generated_batches(n, seed):
    """n small (items, requests): random trees, one-bucket trees, 10-nibble-prefix trees."""
    rng = np.random.default_rng(seed)
    for i in range(n):
        m = int(rng.integers(0, 28))
        ks = _rand(rng, m) if i % 3 == 0 else _under("3d3d" if i % 3 == 1 else "3d3d3d3d3d", rng, m)
        if m and i % 5 == 0:
            near = bytearray(ks[0])
            near[int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
            ks.append(bytes(near))
        items = {k: v for k, v in zip(ks, _rand(rng, len(ks)))}
        yield items, requests_for(items, rng, 12)


# ---- the fixture ----
GOLDEN_CASES = ["one_key", "pair63_third", "seventeen_buckets", "all_modes"]


def golden_document():
    """What tests/golden/shamap_get.json holds: a few cases and their answers;
    written only when the walk and the closed form agree."""
    out = []
    for name in GOLDEN_CASES:
        items, requests, _ = case(name)
        for nid, depth, mode in requests:
            assert answer_by_walk(items, nid, depth, mode) == answer_closed(items, nid, depth, mode), name
        a = Answer(items, requests)
        out.append({"case": name, "root": SM.root_recursive(items)[0].hex(),
                    "items": [[k.hex(), items[k].hex()] for k in sorted(items)],
                    "requests": [[nid.hex(), depth, mode] for nid, depth, mode in requests],
                    "status": a.status, "first": a.first, "rows": a.rows,
                    "leaf_key": [k.hex() for k in a.leaf_key], "counts": a.counts,
                    "nodes": [{"depth": d, "id": nid.hex(), "hash": h.hex(), "leaf_mask": mask}
                              for d, nid, h, _, mask in a.node]})
    return {"answers": out}


# ---- the host emulation ----
def load_get_emu():
    from stellard_amd import build
    build.build_hostemu_shamap_get()
    lib = ctypes.CDLL(GET_SO)
    V, U, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    for name, res, args in (
            ("hostemu_get_id_masked", I, [V, U]),
            ("hostemu_get_kind", U, [U, U, I]),
            ("hostemu_get_path_depth", U, [ctypes.c_int32]),
            ("hostemu_get_path_status", U, [ctypes.c_int32, U]),
            ("hostemu_get_top_index", U, [U, U]),
            ("hostemu_get_scratch_pos", U, [U, U, U]),
            ("hostemu_get_branch_end", U, [V, U, U, U]),
            ("hostemu_get_range", None, [V, V, U, V, U, V, V]),
            ("hostemu_get_bucket_values", None, [V, V, U, V, V]),
            ("hostemu_get_nodes", I, [V, V, V, V, U, V, V, V, U, V, V, V, V, V, U, V, V, V, V, V, V, V])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class EmuResult:
    pass


def emu_get(emu, items, requests, modes=True, max_nodes=None, ids=True, meta=True, leaves=True, total=None):
    """The staged call on a generation of exactly the tree's size -> an EmuResult
    with exactly sized, guarded outputs."""
    g = LM.EmuGen(items)
    n = len(requests)
    rid, rdepth, rmode = request_arrays(requests)
    if max_nodes is None:
        max_nodes = total if total is not None else MAX_ROWS * n
    r = EmuResult()
    r.out = NM.EmuOut(max_nodes, ids, meta)
    r.status = np.full(n + 1, 0xA5, np.uint8)
    r.first = np.full(n + 1, 0xA5A5A5A5, np.uint32)
    r.rows = np.full(n + 1, 0xA5A5A5A5, np.uint32)
    r.leaf_key = np.full((n + 1, 32), 0xA5, np.uint8) if leaves else None
    r.leaf_hash = np.full((n + 1, 32), 0xA5, np.uint8) if leaves else None
    r.counts = np.full(9, 0xA5A5A5A5, np.uint32)
    r.info = np.zeros(2, np.uint32)
    p = LM._p
    rc = emu.hostemu_get_nodes(p(g.key), p(g.leaf), p(g.bcnt), p(g.bh), g.m, p(rid), p(rdepth),
                               p(rmode) if modes else None, n, p(r.status), p(r.first), p(r.rows), p(r.leaf_key),
                               p(r.leaf_hash), *r.out.args(), p(r.counts), p(r.info))
    assert rc == 0, rc
    assert r.status[n] == 0xA5 and r.first[n] == 0xA5A5A5A5 and r.rows[n] == 0xA5A5A5A5 and r.counts[8] == 0xA5A5A5A5
    if leaves:
        assert (r.leaf_key[n] == 0xA5).all() and (r.leaf_hash[n] == 0xA5).all()
    assert r.out.guards_intact()
    return r


def check_emu(ans, r):
    o = r.out
    check_outputs(ans, r.status, r.first, r.rows, r.leaf_key, r.leaf_hash, o.hash, o.body, o.ids, o.meta, o.count[0],
                  r.counts[:8])
