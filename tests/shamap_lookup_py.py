"""The resident SHAMap's read-only calls (stl_shamap_tree_lookup*,
stl_shamap_tree_compare*) in Python: the model the host emulation and the GPU
calls are tested against.  It runs over the dicts {key: leaf hash} of
tests/shamap_tree_py.Model.

lookup(items, keys) -> (found, leaf hashes, positions): per query key whether
the map holds it, its leaf hash (zeros when absent) and its row among the sorted
keys (0xFFFFFFFF when absent).

compare(items_a, items_b, max_rows) -> (rows, counts): the differences in
ascending key order, the first max_rows of them, as (key, kind, leaf in a, leaf
in b), and the eight counts.  The bucket rule is applied through
shamap_tree_py's bucket values: a bucket whose (count, hash) is equal in both
maps is not examined, so counts[4] (buckets examined) and counts[5] (their
items, of a plus of b) are modelled -- and a difference hidden behind equal
bucket values would go unreported here exactly as on the device.

Also the binding of the host emulation (load_lookup_emu) and the pairs of maps
the golden file and the tests share (pair)."""
import ctypes
import os

import numpy as np

from tests import shamap_tree_py as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOKUP_SO = os.path.join(ROOT, "tests", "native", "libhostemu_shamap_lookup.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "shamap_compare.json")
A_ONLY, B_ONLY, CHANGED = 1, 2, 3
NO_ROW = 0xFFFFFFFF
ZERO = bytes(32)


def lookup(items, keys):
    order = {k: i for i, k in enumerate(sorted(items))}
    found, leaf, pos = [], [], []
    for k in keys:
        k = bytes(k)
        found.append(k in items)
        leaf.append(items.get(k, ZERO))
        pos.append(order.get(k, NO_ROW))
    return found, leaf, pos


def by_bucket(items):
    out = {}
    for k, v in items.items():
        out.setdefault(TM.bucket(k), {})[k] = v
    return out


def bucket_value(sub, b):
    """(count, hash) of bucket b over its own items, by shamap_tree_py's recurrence."""
    return TM.prefix_value(sub, "%04x" % b)


def bucket_differs(sub_a, sub_b, b):
    if sub_a == sub_b:  # the same content has the same value: nothing to hash
        return False
    return bucket_value(sub_a, b) != bucket_value(sub_b, b)


def compare(items_a, items_b, max_rows):
    ba, bb = by_bucket(items_a), by_bucket(items_b)
    rows, kinds, buckets, examined = [], [0, 0, 0, 0], 0, 0
    for b in sorted(set(ba) | set(bb)):
        sa, sb = ba.get(b, {}), bb.get(b, {})
        if not bucket_differs(sa, sb, b):
            continue
        buckets += 1
        examined += len(sa) + len(sb)
        for k in sorted(set(sa) | set(sb)):
            if k not in sb:
                row = (k, A_ONLY, sa[k], ZERO)
            elif k not in sa:
                row = (k, B_ONLY, ZERO, sb[k])
            elif sa[k] != sb[k]:
                row = (k, CHANGED, sa[k], sb[k])
            else:
                continue
            kinds[row[1]] += 1
            rows.append(row)
    counts = [len(rows), kinds[A_ONLY], kinds[B_ONLY], kinds[CHANGED], buckets, examined, len(items_a), len(items_b)]
    return rows[:max_rows], counts


def brute_compare(items_a, items_b):
    """The differences without any bucket rule."""
    rows = []
    for k in sorted(set(items_a) | set(items_b)):
        va, vb = items_a.get(k), items_b.get(k)
        if va != vb:
            rows.append((k, A_ONLY if vb is None else B_ONLY if va is None else CHANGED, va or ZERO, vb or ZERO))
    return rows


# ---- the shared pairs of maps ----
def _partner(key, shared, rng):
    hx = key.hex()
    other = "%x" % (int(hx[shared], 16) ^ (1 + int(rng.integers(0, 15))))
    tail = rng.integers(0, 256, 32, dtype=np.uint8).tobytes().hex()[shared + 1:]
    return bytes.fromhex(hx[:shared] + other + tail)


def _rand(rng, n=1):
    return [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]


def derive(items, rng, only_a=0, only_b=0, changed=0):
    """-> (a, b): a = items; b = items with `only_a` keys removed, `only_b` new
    keys added and `changed` leaf hashes replaced."""
    ks = sorted(items)
    pick = [ks[int(i)] for i in rng.permutation(len(ks))[:only_a + changed]]
    b = dict(items)
    for k in pick[:only_a]:
        del b[k]
    for k in pick[only_a:]:
        b[k] = _rand(rng)[0]
    for k in _rand(rng, only_b):
        b[k] = _rand(rng)[0]
    return dict(items), b


PAIRS = ["empty", "self", "vs_empty", "empty_vs", "one_of_each", "bucket_1_1", "bucket_1_2", "shared_3_4_63", "mixed300"]


def pair(name):
    """A seeded pair of maps ({key: leaf}, {key: leaf}) by name."""
    rng = np.random.default_rng(700 + PAIRS.index(name))
    base = {k: v for k, v in zip(_rand(rng, 40), _rand(rng, 40))}
    if name == "empty":
        return {}, {}
    if name == "self":
        return base, dict(base)
    if name == "vs_empty":
        return base, {}
    if name == "empty_vs":
        return {}, base
    if name == "one_of_each":
        return derive(base, rng, 1, 1, 1)
    if name == "bucket_1_1":  # a 1-key bucket against a 1-key bucket with another key
        k = _rand(rng)[0]
        other = _partner(k, 10, rng)
        return {**base, k: k}, {**base, other: other}  # a leaf hash commits to its key: never k's under another key
    if name == "bucket_1_2":  # a 1-key bucket against a 2-key bucket
        k = _rand(rng)[0]
        return {**base, k: k}, {**base, k: k, _partner(k, 7, rng): ZERO[:31] + b"\x01"}
    if name == "shared_3_4_63":
        a, b = dict(base), dict(base)
        for shared in (3, 4, 63):
            k = _rand(rng)[0]
            other = _partner(k, shared, rng)
            a[k] = k
            b[other] = other
        return a, b
    if name == "mixed300":
        big = {k: v for k, v in zip(_rand(rng, 300), _rand(rng, 300))}
        return derive(big, rng, 20, 30, 25)
    raise KeyError(name)


def arrays(items):
    """(keys, leaf hashes) as (m, 32) uint8 arrays, in insertion order."""
    a = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 32).copy()  # noqa: E731
    return a(list(items)), a(list(items.values()))


# ---- the host emulation ----
def load_lookup_emu():
    from stellard_amd import build
    build.build_hostemu_shamap_lookup()
    lib = ctypes.CDLL(LOOKUP_SO)
    V, U = ctypes.c_void_p, ctypes.c_uint32
    for name, res, args in (
            ("hostemu_lookup_range", None, [U, U, U, V, V]),
            ("hostemu_lookup_lower_bound", U, [V, U, U, V, V]),
            ("hostemu_bucket_differs", ctypes.c_int, [U, V, U, V]),
            ("hostemu_diff_rank_a", U, [U, U]),
            ("hostemu_diff_rank_b", U, [U, U]),
            ("hostemu_diff_kind_a", U, [ctypes.c_int, ctypes.c_int]),
            ("hostemu_diff_kind_b", U, [ctypes.c_int]),
            ("hostemu_diff_bucket_of", U, [V, U]),
            ("hostemu_diff_slot", U, [V, V, U, U, V, V, U, U, U, V, V, V]),
            ("hostemu_lookup", None, [V, V, V, U, V, U, V, V, V]),
            ("hostemu_compare", ctypes.c_int, [V, V, V, V, U, V, V, V, V, U, U, V, V, V, V, V])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class EmuGen:
    """One generation on host arrays: sorted keys, leaf hashes, bucket counts
    and bucket hashes (from shamap_tree_py's recurrence)."""

    def __init__(self, items):
        ks = sorted(items)
        self.m = len(ks)
        self.key = np.frombuffer(b"".join(ks), np.uint8).copy() if ks else np.zeros(0, np.uint8)
        self.leaf = np.frombuffer(b"".join(items[k] for k in ks), np.uint8).copy() if ks else np.zeros(0, np.uint8)
        self.bcnt = np.zeros(TM.BUCKETS, np.uint32)
        self.bh = np.zeros((TM.BUCKETS, 32), np.uint8)
        for b, sub in by_bucket(items).items():
            cnt, h = bucket_value(sub, b)
            self.bcnt[b] = cnt
            self.bh[b] = np.frombuffer(h, np.uint8)


def emu_lookup(emu, gen, keys):
    n = len(keys)
    q = np.frombuffer(b"".join(bytes(k) for k in keys), np.uint8).copy() if n else np.zeros(0, np.uint8)
    words = np.full((n + 63) // 64 + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    leaf = np.full((n, 32), 0xA5, np.uint8)
    pos = np.full(n, 0xA5A5A5A5, np.uint32)
    emu.hostemu_lookup(_p(gen.key), _p(gen.leaf), _p(gen.bcnt), gen.m, _p(q), n, _p(words), _p(leaf), _p(pos))
    assert words[-1] == 0xA5A5A5A5A5A5A5A5  # nothing past ceil(n / 64) words
    bits = np.unpackbits(words[:-1].view(np.uint8), bitorder="little")
    assert not bits[n:].any()  # the tail bits are zero
    return [bool(x) for x in bits[:n]], [r.tobytes() for r in leaf], [int(x) for x in pos]


def emu_compare(emu, ga, gb, max_rows, leaves=True):
    rows = max(max_rows, 1)
    key = np.full((rows + 1, 32), 0xA5, np.uint8)
    kind = np.full(rows + 1, 0xA5, np.uint8)
    la = np.full((rows + 1, 32), 0xA5, np.uint8) if leaves else None
    lb = np.full((rows + 1, 32), 0xA5, np.uint8) if leaves else None
    counts = np.zeros(8, np.uint32)
    rc = emu.hostemu_compare(_p(ga.key), _p(ga.leaf), _p(ga.bcnt), _p(ga.bh), ga.m, _p(gb.key), _p(gb.leaf), _p(gb.bcnt),
                        _p(gb.bh), gb.m, max_rows, _p(key), _p(kind), _p(la), _p(lb), _p(counts))
    assert rc == 0, rc  # every slot of every examined bucket written exactly once
    c = [int(x) for x in counts]
    r = min(c[0], max_rows)
    for arr in (key, kind, la, lb):  # exactly min(|D|, max_rows) rows are written
        assert arr is None or (arr[r:] == 0xA5).all()
    out = [(key[i].tobytes(), int(kind[i]), la[i].tobytes() if leaves else None, lb[i].tobytes() if leaves else None)
           for i in range(r)]
    return out, c
