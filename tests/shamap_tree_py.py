"""The resident SHAMap (stl_shamap_tree_*) in Python: the model the host
emulation and the GPU calls are tested against.

A tree is a dict {key: leaf hash}.  A batch reads as a sequence of changes:
of rows with equal keys the last one counts; a set inserts or replaces, a
delete removes.  The root is shamap_py.model's over the resulting set -- the
model knows nothing of buckets, generations or merges.  The eight counts:
items after, inserted, replaced, deleted, deletes of absent keys, rows
superseded by a later row, dirty buckets (the 4-nibble prefixes of the changes'
keys) and leaves gathered (the items of the dirty buckets afterwards).

Also the bucket recurrence stated on its own (root_by_buckets), the seeded
batch sequences the tests share (sequence) and the binding of the host
emulation (load_tree_emu)."""
import ctypes
import os

import numpy as np

from tests import shamap_py as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_SO = os.path.join(ROOT, "tests", "native", "libhostemu_shamap_tree.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "shamap_tree_roots.json")
BUCKET_DEPTH = 4
BUCKETS = 1 << 16


def bucket(key):
    return (key[0] << 8) | key[1]


def delta(is_delete, found):
    if is_delete:
        return -1 if found else 0
    return 0 if found else 1


class Model:
    def __init__(self):
        self.items = {}

    def apply(self, keys, leaf_hashes=None, ops=None):
        """One batch -> (root, [8 counts])."""
        n = len(keys)
        last = {}
        for i in range(n):
            last[bytes(keys[i])] = i
        ins = rep = dele = absent = 0
        dirty = set()
        for k, i in last.items():
            is_del = ops is not None and bool(ops[i])
            found = k in self.items
            dirty.add(bucket(k))
            if is_del:
                if found:
                    del self.items[k]
                    dele += 1
                else:
                    absent += 1
            else:
                self.items[k] = k if leaf_hashes is None else bytes(leaf_hashes[i])
                if found:
                    rep += 1
                else:
                    ins += 1
        gathered = sum(1 for k in self.items if bucket(k) in dirty)
        return self.root(), [len(self.items), ins, rep, dele, absent, n - len(last), len(dirty), gathered]

    def root(self):
        ks = sorted(self.items)
        if not ks:
            return SM.ZERO
        return SM.model(np.frombuffer(b"".join(ks), np.uint8).reshape(-1, 32),
                        np.frombuffer(b"".join(self.items[k] for k in ks), np.uint8).reshape(-1, 32))[0]

    def content(self):
        """(keys, leaf hashes) sorted, as (m, 32) uint8 arrays."""
        ks = sorted(self.items)
        a = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 32).copy()  # noqa: E731
        return a(ks), a([self.items[k] for k in ks])


# ---- the recurrence, stated on its own ----
def prefix_value(items, prefix_hex):
    """(cnt, h) of a nibble prefix over {key: leaf hash}: h zero for no key, the
    one key's leaf hash for one, the inner node's hash at (len, prefix) for more."""
    under = {k: v for k, v in items.items() if k.hex().startswith(prefix_hex)}
    if not under:
        return 0, SM.ZERO
    if len(under) == 1:
        return 1, next(iter(under.values()))
    d = len(prefix_hex)
    slots = [prefix_value(under, prefix_hex + c)[1] for c in "0123456789abcdef"] if d < 63 else \
        [next((v for k, v in under.items() if k.hex()[63] == c), SM.ZERO) for c in "0123456789abcdef"]
    return len(under), SM.inner_hash(slots)


def root_by_buckets(items):
    """The root from the values of the 16 depth-1 prefixes (an inner node whenever a key exists)."""
    if not items:
        return SM.ZERO
    return SM.inner_hash([prefix_value(items, c)[1] for c in "0123456789abcdef"])


# ---- the shared batch sequences ----
def _mixed_batch(rng, model_keys, rows):
    """rows rows: sets of new keys, replaces and deletes of resident ones,
    deletes of absent keys, and repeated keys whose rows disagree."""
    res = list(model_keys)
    keys = rng.integers(0, 256, (rows, 32), dtype=np.uint8)
    ops = np.zeros(rows, np.uint8)
    kind = rng.integers(0, 8, rows)
    for i in range(rows):
        if res and kind[i] in (0, 1, 2):  # replace
            keys[i] = np.frombuffer(res[int(rng.integers(0, len(res)))], np.uint8)
        elif res and kind[i] in (3, 4):  # delete
            keys[i] = np.frombuffer(res[int(rng.integers(0, len(res)))], np.uint8)
            ops[i] = 1
        elif kind[i] == 5:  # delete of an absent key
            ops[i] = 1 + int(rng.integers(0, 255))
        elif kind[i] == 6 and i:  # a repeated key: an earlier row's, with its own op
            keys[i] = keys[int(rng.integers(0, i))]
            ops[i] = int(rng.integers(0, 2))
    return keys, rng.integers(0, 256, (rows, 32), dtype=np.uint8), ops


def sequence(name):
    """A seeded sequence of batches [(keys, leaf hashes or None, ops or None)]
    from an empty tree, by name."""
    seed = {"small": 101, "mixed": 102, "clustered": 103, "drain": 104}[name]
    rng = np.random.default_rng(seed)
    m, out = Model(), []

    def push(b):
        out.append(b)
        m.apply(*b)

    if name == "small":
        k = SM.case_keys("random40", seed)
        push((k[:1], None, None))
        push((k[1:17], k[1:17][:, ::-1].copy(), None))
        for rows in (1, 7, 33):
            push(_mixed_batch(rng, m.items, rows))
    elif name == "mixed":
        k = SM.case_keys("random600", seed)
        push((k, rng.integers(0, 256, k.shape, dtype=np.uint8), np.zeros(600, np.uint8)))
        for rows in (1, 300, 64, 257):
            push(_mixed_batch(rng, m.items, rows))
    elif name == "clustered":
        k = SM.case_keys("cluster500_3_62", seed)  # three buckets hold everything, down to depth 62
        push((k, None, None))
        more = SM.case_keys("cluster200_3_62", seed)  # the same heads: the seed fixes them
        push((more, rng.integers(0, 256, more.shape, dtype=np.uint8), None))
        push(_mixed_batch(rng, m.items, 150))
        push((k[::2].copy(), None, np.ones(250, np.uint8)))
    elif name == "drain":
        k = SM.case_keys("random300", seed)
        push((k, None, None))
        push((k[:299].copy(), None, np.ones(299, np.uint8)))  # one key left
        push((k[299:].copy(), None, np.ones(1, np.uint8)))    # none
        push((k[:5].copy(), None, None))
    return out


SEQUENCES = ["small", "mixed", "clustered", "drain"]


def run_sequence(name):
    """-> [(root, counts)] after every step, by the model."""
    m = Model()
    return [m.apply(*b) for b in sequence(name)]


# ---- the host emulation ----
def load_tree_emu():
    from stellard_amd import build
    build.build_hostemu_shamap_tree()
    lib = ctypes.CDLL(TREE_SO)
    V, U, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    for name, res, args in (
            ("hostemu_tree_bucket", U, [V]),
            ("hostemu_tree_head", ctypes.c_int, [ctypes.c_int, U]),
            ("hostemu_tree_delta", I, [ctypes.c_int, ctypes.c_int]),
            ("hostemu_tree_item_dest", U, [U, U]),
            ("hostemu_tree_insert_dest", U, [U, U]),
            ("hostemu_tree_changes_before", U, [V, V, U, U, V]),
            ("hostemu_tree_lower_bound", U, [V, U, V, V]),
            ("hostemu_tree_bucket_begin", U, [V, U, U]),
            ("hostemu_tree_top_value", U, [V, V, ctypes.c_int, V]),
            ("hostemu_tree_new", V, [U]),
            ("hostemu_tree_free", None, [V]),
            ("hostemu_tree_apply", ctypes.c_int, [V, V, V, V, U, V, V]),
            ("hostemu_tree_export", U, [V, V, V])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class EmuTree:
    """The staged apply of tests/native/hostemu_shamap_tree.cpp on host arrays."""

    def __init__(self, emu, capacity):
        self.emu, self.capacity = emu, capacity
        self.h = emu.hostemu_tree_new(capacity)

    def apply(self, keys, leaf_hashes=None, ops=None):
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
        leaf = None if leaf_hashes is None else np.ascontiguousarray(leaf_hashes, np.uint8)
        op = None if ops is None else np.ascontiguousarray(ops, np.uint8)
        root, cnt = np.zeros(32, np.uint8), np.zeros(8, np.uint32)
        rc = self.emu.hostemu_tree_apply(self.h, p(keys), p(leaf), p(op), keys.shape[0], p(root), p(cnt))
        return rc, root.tobytes(), [int(x) for x in cnt]

    def content(self):
        k = np.zeros((self.capacity, 32), np.uint8)
        l = np.zeros((self.capacity, 32), np.uint8)
        m = self.emu.hostemu_tree_export(self.h, k.ctypes.data_as(ctypes.c_void_p), l.ctypes.data_as(ctypes.c_void_p))
        return k[:m], l[:m]

    def close(self):
        if self.h:
            self.emu.hostemu_tree_free(self.h)
            self.h = None
