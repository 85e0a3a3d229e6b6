"""The SHAMap root of a set of 32-byte keys, in Python: the model the host
emulation and the GPU calls (stl_shamap_root*) are tested against.

Two independent statements of one function of the set:

  * root_recursive: the definition over the sorted set -- the node at depth d
    over the keys that share d nibbles has one branch per nibble d; a branch
    with one key is that key's leaf, with more an inner node one level down;
    the root is an inner node whatever it holds;
  * root_by_insertion: a tree grown item by item the way a node grows its own
    (walk down by nibbles; an empty branch takes the leaf; a leaf in the way
    becomes a chain of inner nodes down to the depth where the two keys part;
    an item whose key is present is refused), hashed afterwards.

Both return (root, inner nodes, deepest inner node's depth).  neighbours(),
counts() and depth_histogram() are the closed forms the device code uses, from
the common nibble prefixes of neighbouring keys.

Also the seeded key sets the tests share (case_keys) and the binding of the
host emulation (load_shamap_emu)."""
import bisect
import ctypes
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAMAP_SO = os.path.join(ROOT, "tests", "native", "libhostemu_shamap.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "shamap_roots.json")

ZERO = bytes(32)
INNER_PREFIX = b"MIN\0"
MAX_ITEMS = 1 << 24


def inner_hash(slots):
    """slots: 16 hashes of 32 bytes (ZERO: empty) -> the inner node's hash."""
    assert len(slots) == 16 and all(len(s) == 32 for s in slots)
    return hashlib.sha512(INNER_PREFIX + b"".join(slots)).digest()[:32]


def nibble(key, d):
    b = key[d >> 1]
    return b & 15 if d & 1 else b >> 4


def common_prefix(a, b):
    """Leading nibbles a and b share: 0 .. 64."""
    for i in range(32):
        x = a[i] ^ b[i]
        if x:
            return 2 * i + (0 if x & 0xF0 else 1)
    return 64


def the_set(keys, leaf_hashes=None, select=None):
    """Rows -> {key: leaf hash}: the selected rows; of equal keys the lowest
    row supplies the leaf hash.  Also the number of selected rows."""
    items, nsel = {}, 0
    for i, k in enumerate(keys):
        if select is not None and not select[i]:
            continue
        nsel += 1
        k = bytes(k)
        if k not in items:
            items[k] = k if leaf_hashes is None else bytes(leaf_hashes[i])
    return items, nsel


# ---- 1. the recursive definition ----
def root_recursive(items):
    """items: {key: leaf hash} -> (root, inner nodes, deepest depth)."""
    if not items:
        return ZERO, 0, 0
    keys = sorted(items)
    hexes = [k.hex() for k in keys]
    stats = [0, 0]

    def node(lo, hi, d):
        stats[0] += 1
        stats[1] = max(stats[1], d)
        prefix = hexes[lo][:d]
        slots = []
        at = lo
        for c in "0123456789abcdef":
            end = bisect.bisect_left(hexes, prefix + chr(ord(c) + 1), at, hi) if c != "f" else hi
            if end == at:
                slots.append(ZERO)
            elif end == at + 1:
                slots.append(items[keys[at]])
            else:
                slots.append(node(at, end, d + 1))
            at = end
        return inner_hash(slots)

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 1000))
    return node(0, len(keys), 0), stats[0], stats[1]


# ---- 2. the insertion walk ----
class _Inner:
    __slots__ = ("child",)

    def __init__(self):
        self.child = [None] * 16


class _Leaf:
    __slots__ = ("key", "hash")

    def __init__(self, key, h):
        self.key, self.hash = key, h


def insert(root, key, h):
    """Adds (key, h) to the tree under `root` (an _Inner); False when the key
    is there already."""
    node, d = root, 0
    while True:
        b = nibble(key, d)
        nxt = node.child[b]
        if nxt is None:
            node.child[b] = _Leaf(key, h)
            return True
        if isinstance(nxt, _Inner):
            node, d = nxt, d + 1
            continue
        if nxt.key == key:
            return False
        # a leaf in the way: inner nodes down to where the two keys part
        other = nxt
        cur = _Inner()
        node.child[b] = cur
        d += 1
        while nibble(key, d) == nibble(other.key, d):
            deeper = _Inner()
            cur.child[nibble(key, d)] = deeper
            cur, d = deeper, d + 1
        cur.child[nibble(key, d)] = _Leaf(key, h)
        cur.child[nibble(other.key, d)] = other
        return True


def hash_tree(root):
    """-> (root hash, inner nodes, deepest depth); iterative post-order."""
    if all(c is None for c in root.child):
        return ZERO, 0, 0
    nodes, deepest = 0, 0
    done = {}
    stack = [(root, 0, False)]
    while stack:
        n, d, seen = stack.pop()
        if not seen:
            stack.append((n, d, True))
            for c in n.child:
                if isinstance(c, _Inner):
                    stack.append((c, d + 1, False))
            continue
        nodes += 1
        deepest = max(deepest, d)
        slots = []
        for c in n.child:
            if c is None:
                slots.append(ZERO)
            elif isinstance(c, _Leaf):
                slots.append(c.hash)
            else:
                slots.append(done.pop(id(c)))
        done[id(n)] = inner_hash(slots)
    return done[id(root)], nodes, deepest


def root_by_insertion(rows):
    """rows: (key, leaf hash) in insertion order -> (root, inner nodes,
    deepest depth, refused rows)."""
    root, refused = _Inner(), 0
    for k, h in rows:
        if not insert(root, bytes(k), bytes(h)):
            refused += 1
    return hash_tree(root) + (refused,)


# ---- the closed forms ----
def neighbours(sorted_keys):
    """l_i for the distinct sorted keys: -1 .. 63; for one key, [0]."""
    m = len(sorted_keys)
    if m == 1:
        return [0]
    return [common_prefix(sorted_keys[i], sorted_keys[i + 1]) if i + 1 < m else -1 for i in range(m)]


def depth_histogram(sorted_keys):
    """Inner nodes per depth: key i starts one at every d with l_{i-1} < d <= l_i."""
    hist = [0] * 64
    lp = -1
    for lc in neighbours(sorted_keys):
        for d in range(lp + 1, lc + 1):
            hist[d] += 1
        lp = lc
    return hist


def counts(keys, select=None):
    """The four counts of stl_shamap_root for these rows."""
    items, nsel = the_set(keys, None, select)
    hist = depth_histogram(sorted(items))
    deep = max((d for d in range(64) if hist[d]), default=0)
    return [len(items), nsel - len(items), sum(hist), deep]


def model(keys, leaf_hashes=None, select=None):
    """Rows -> (root, counts) by the recursive definition, the counts by the
    closed forms; the two must agree on nodes and depth."""
    items, nsel = the_set(keys, leaf_hashes, select)
    root, nodes, deep = root_recursive(items)
    c = counts(keys, select)
    assert c == [len(items), nsel - len(items), nodes, deep], (c, nodes, deep)
    return root, c


# ---- the shared key sets ----
def _rows(a):
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 32)


def case_keys(shape, seed):
    """A seeded key set, (n, 32) uint8, by shape name:
    randomN; clusterN_C_P (N keys in C clusters sharing P nibbles);
    deepest (two keys that part at the last nibble); dense (4,096 keys sharing
    60 nibbles); root17 (all 16 root branches and one collision); multiword
    (keys equal in their first 8, 16, 24 bytes, among random ones);
    dupsN (N random keys, a quarter of them repeated, shuffled)."""
    rng = np.random.default_rng(seed)
    if shape.startswith("random"):
        return _rows(rng.integers(0, 256, (int(shape[6:]), 32), dtype=np.uint8))
    if shape.startswith("cluster"):
        n, c, p = (int(x) for x in shape[7:].split("_"))
        heads = rng.integers(0, 256, (c, 32), dtype=np.uint8)
        k = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        which = rng.integers(0, c, n)
        full = p // 2
        k[:, :full] = heads[which, :full]
        if p & 1:
            k[:, full] = (heads[which, full] & 0xF0) | (k[:, full] & 0x0F)
        return _rows(k)
    if shape == "deepest":
        k = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), 2, axis=0)
        k[0, 31] = (k[0, 31] & 0xF0) | 0x3
        k[1, 31] = (k[1, 31] & 0xF0) | 0xC
        return _rows(k)
    if shape == "dense":
        k = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), 4096, axis=0)
        tail = rng.permutation(65536)[:4096]  # the last four nibbles, distinct
        k[:, 30] = tail >> 8
        k[:, 31] = tail & 0xFF
        return _rows(k)
    if shape == "root17":
        k = rng.integers(0, 256, (17, 32), dtype=np.uint8)
        for b in range(16):
            k[b, 0] = (b << 4) | (k[b, 0] & 0x0F)
        k[16, 0] = k[5, 0]  # shares the root branch and the second nibble with key 5
        return _rows(k)
    if shape == "multiword":
        k = rng.integers(0, 256, (96, 32), dtype=np.uint8)
        for j, cut in enumerate((8, 16, 24)):
            k[8 * j: 8 * j + 8, :cut] = k[8 * j, :cut]
        # the keys with a common head differ in the byte after it and later,
        # in an order unlike their row order
        return _rows(k[rng.permutation(96)])
    if shape.startswith("dups"):
        n = int(shape[4:])
        k = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        k[3 * n // 4:] = k[rng.integers(0, 3 * n // 4, n - 3 * n // 4)]
        return _rows(k[rng.permutation(n)])
    raise ValueError(shape)


# (shape, seed) of tests/golden/shamap_roots.json (tests/golden/make_shamap.py writes it)
GOLDEN_CASES = [("random1", 1), ("random2", 2), ("root17", 3), ("deepest", 4), ("dense", 5), ("multiword", 6),
                ("random63", 7), ("random257", 8), ("random4097", 9), ("cluster4096_16_40", 10), ("dups1000", 11),
                ("cluster300_3_63", 12)]


def load_shamap_emu():
    from stellard_amd import build
    build.build_hostemu_shamap()
    lib = ctypes.CDLL(SHAMAP_SO)
    V, U, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    for name, res, args in (
            ("hostemu_shamap_nibble", U, [V, U]),
            ("hostemu_shamap_common_prefix", U, [V, V]),
            ("hostemu_shamap_key_less", ctypes.c_int, [V, V]),
            ("hostemu_shamap_sort_word", ctypes.c_uint64, [V, U]),
            ("hostemu_shamap_neighbour", I, [V, V, ctypes.c_int, ctypes.c_int]),
            ("hostemu_shamap_starts_node", ctypes.c_int, [I, I, I]),
            ("hostemu_shamap_leaf_parent_depth", I, [I, I]),
            ("hostemu_shamap_inner_hash", None, [V, V]),
            ("hostemu_shamap_range_end", U, [V, U, U, U]),
            ("hostemu_shamap_branch_first", U, [V, U, U, U, U]),
            ("hostemu_shamap_root", ctypes.c_int, [V, V, V, U, V, V, V, V])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def emu_root(emu, keys, leaf_hashes=None, select=None):
    """The host emulation's whole computation -> (root, counts, histogram, l)."""
    keys = _rows(keys)
    n = keys.shape[0]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    leaf = None if leaf_hashes is None else _rows(leaf_hashes)
    sel = None if select is None else np.packbits(np.asarray(select, dtype=bool), bitorder="little")
    root = np.zeros(32, np.uint8)
    cnt = np.zeros(4, np.uint32)
    hist = np.zeros(64, np.uint32)
    l = np.full(max(n, 1), -2, np.int8)
    assert emu.hostemu_shamap_root(p(keys), p(leaf), p(sel), n, p(root), p(cnt), p(hist), p(l)) == 0
    return root.tobytes(), [int(x) for x in cnt], [int(x) for x in hist], [int(x) for x in l[:cnt[0]]]
