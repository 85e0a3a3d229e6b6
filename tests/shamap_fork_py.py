"""The resident SHAMap's fork and revert in Python: what the host emulation and
the GPU calls are tested against.

A fork is the model of tests/shamap_tree_py.py copied, then applied: the
source's dict stays, the destination's becomes the copy with the batch.  A
revert is the dict the tree held before its last successful apply or fork --
one step, and none after a call that failed (ModelTree).

Also the small seeded cases that tests/golden/shamap_fork.json pins (cases) and
the binding of tests/native/hostemu_shamap_fork.cpp (load_fork_emu, EmuTree)."""
import ctypes
import os

import numpy as np

from tests import shamap_py as SM
from tests import shamap_tree_py as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORK_SO = os.path.join(ROOT, "tests", "native", "libhostemu_shamap_fork.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "shamap_fork.json")
EINVAL = -3  # the emulation's code where the C calls give STL_EINVAL


def fork(src, keys=None, leaf_hashes=None, ops=None):
    """The model: src (a TM.Model) copied, then applied -> (the new Model, root,
    [8 counts]).  src is not touched."""
    dst = TM.Model()
    dst.items = dict(src.items)
    if keys is None or len(keys) == 0:
        return dst, dst.root(), [len(dst.items)] + [0] * 7
    root, counts = dst.apply(keys, leaf_hashes, ops)
    return dst, root, counts


class ModelTree:
    """A tree with the one-step revert: the content, and what a revert gives
    back (None: a revert is refused)."""

    def __init__(self, capacity):
        self.capacity, self.m, self.prev = capacity, TM.Model(), None

    def _take(self, new):
        if len(new.items) > self.capacity:
            self.prev = None  # a call that failed past its checks: no revert until the next good one
            return False
        self.prev, self.m = self.m, new
        return True

    def apply(self, keys, leaf_hashes=None, ops=None):
        if len(keys) == 0:
            return True  # changes nothing, the revert state included
        return self._take(fork(self.m, keys, leaf_hashes, ops)[0])

    def fork_from(self, src, keys=None, leaf_hashes=None, ops=None):
        return self._take(fork(src.m, keys, leaf_hashes, ops)[0])

    def revert(self):
        if self.prev is None:
            return False
        self.m, self.prev = self.prev, None
        return True


def difference(a, b):
    """The compare of two dicts -> (only in a, only in b, in both with another leaf hash)."""
    return (sum(1 for k in a if k not in b), sum(1 for k in b if k not in a),
            sum(1 for k in a if k in b and a[k] != b[k]))


# ---- the small cases the golden file pins ----
CASES = ["snapshot_empty", "snapshot_one", "snapshot_300", "mixed_batch", "one_bucket", "collapse_2_to_1",
         "empties_the_tree", "bucket_boundary"]


def case(name):
    """-> (source Model, (keys, leaf hashes or None, ops or None))."""
    rng = np.random.default_rng(2100 + CASES.index(name))
    src = TM.Model()
    none = (np.zeros((0, 32), np.uint8), None, None)
    if name == "snapshot_empty":
        return src, none
    if name == "snapshot_one":
        src.apply(SM.case_keys("random1", 5))
        return src, none
    k = SM.case_keys("random300", 6)
    if name == "snapshot_300":
        src.apply(k, k[:, ::-1].copy())
        return src, none
    if name == "mixed_batch":
        src.apply(k, k[:, ::-1].copy())
        return src, TM._mixed_batch(rng, src.items, 97)
    if name == "one_bucket":
        c = SM.case_keys("cluster200_1_40", 7)
        src.apply(c[:150])
        return src, (c[100:].copy(), rng.integers(0, 256, (100, 32), dtype=np.uint8),
                     (np.arange(100) % 3 == 0).astype(np.uint8))
    if name == "collapse_2_to_1":
        src.apply(k[:2])
        return src, (k[:1].copy(), None, np.ones(1, np.uint8))
    if name == "empties_the_tree":
        src.apply(k[:40])
        return src, (k[:40].copy(), None, np.ones(40, np.uint8))
    if name == "bucket_boundary":
        a = k[0].copy()
        b3, b4 = a.copy(), a.copy()
        b3[1] ^= 0x01  # shares 3 nibbles with a: the neighbouring bucket
        b4[2] ^= 0x10  # shares 4: the same bucket, parted one level below it
        src.apply(np.stack([a, b3]))
        return src, (np.stack([b4, b3]), None, np.array([0, 1], np.uint8))
    raise KeyError(name)


# ---- the host emulation ----
def load_fork_emu():
    from stellard_amd import build
    build.build_hostemu_shamap_fork()
    lib = ctypes.CDLL(FORK_SO)
    V, U = ctypes.c_void_p, ctypes.c_uint32
    for name, res, args in (
            ("hostemu_fork_readable", U, [U, U]),
            ("hostemu_fork_snapshot_rows", U, [U, U, U]),
            ("hostemu_fork_new", V, [U]),
            ("hostemu_fork_free", None, [V]),
            ("hostemu_fork_export", U, [V, V, V, V]),
            ("hostemu_fork_state_count", None, [V, U]),
            ("hostemu_fork_apply", ctypes.c_int, [V, V, V, V, U, V, V]),
            ("hostemu_fork_fork", ctypes.c_int, [V, V, V, V, V, U, V, V]),
            ("hostemu_fork_revert", ctypes.c_int, [V])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def _batch(keys, leaf_hashes, ops):
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    keys = np.zeros((0, 32), np.uint8) if keys is None else np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
    leaf = None if leaf_hashes is None else np.ascontiguousarray(leaf_hashes, np.uint8)
    op = None if ops is None else np.ascontiguousarray(ops, np.uint8)
    root, cnt = np.zeros(32, np.uint8), np.zeros(8, np.uint32)
    return (keys, leaf, op, root, cnt), (p(keys), p(leaf), p(op), keys.shape[0], p(root), p(cnt))


class EmuTree:
    """A tree of tests/native/hostemu_shamap_fork.cpp: exactly sized host arrays."""

    def __init__(self, emu, capacity):
        self.emu, self.capacity = emu, capacity
        self.h = emu.hostemu_fork_new(capacity)

    def apply(self, keys, leaf_hashes=None, ops=None):
        keep, args = _batch(keys, leaf_hashes, ops)
        rc = self.emu.hostemu_fork_apply(self.h, *args)
        return rc, keep[3].tobytes(), [int(x) for x in keep[4]]

    def fork(self, dst, keys=None, leaf_hashes=None, ops=None):
        keep, args = _batch(keys, leaf_hashes, ops)
        rc = self.emu.hostemu_fork_fork(self.h, dst.h, *args)
        return rc, keep[3].tobytes(), [int(x) for x in keep[4]]

    def revert(self):
        return self.emu.hostemu_fork_revert(self.h)

    def state_count(self, count):
        self.emu.hostemu_fork_state_count(self.h, count)

    def content(self):
        """-> (keys, leaf hashes, root, the stated count)."""
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        k = np.zeros((self.capacity, 32), np.uint8)
        l = np.zeros((self.capacity, 32), np.uint8)
        root = np.zeros(32, np.uint8)
        m = self.emu.hostemu_fork_export(self.h, p(k), p(l), p(root))
        rows = min(m, self.capacity)
        return k[:rows].tobytes(), l[:rows].tobytes(), root.tobytes(), m

    def close(self):
        if self.h:
            self.emu.hostemu_fork_free(self.h)
            self.h = None


def content_of(model):
    """A Model's content as EmuTree.content gives it."""
    k, l = model.content()
    return k.tobytes(), l.tobytes(), model.root(), len(model.items)
