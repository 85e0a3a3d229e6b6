"""The resident SHAMap on the host: the model of tests/shamap_tree_py.py against
itself and against stellard_amd/csrc/stl_shamap_tree_core.h compiled for the
host by tests/native/hostemu_shamap_tree.cpp.

  * the model's root (shamap_py.model over the resulting set) equals the bucket
    recurrence stated on its own, also on pairs of keys that share exactly 3, 4
    and 63 nibbles,
  * each rule of the core header equals the model's function: the bucket of a
    key, the head rule, the delta, the two position formulas, the search for
    the changes before an item, the bisections, the top recurrence,
  * the whole staged apply (steps 1-7 on host arrays) equals the model over the
    shared sequences, the golden file and the shapes of tests/shamap_py.py,
  * tests/golden/shamap_tree_roots.json pins the model,
  * the same code in a stand-alone ASan + UBSan program (never loaded into Python),
  * the entry points' argument checks where there is no GPU, and the Python
    wrapper's dtype and shape checks."""
import ctypes
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import shamap_py as SM
from tests import shamap_tree_py as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SHAPES = [("random1", 2), ("random2", 3), ("random17", 4), ("random300", 5), ("random5000", 6), ("root17", 7),
          ("deepest", 8), ("dense", 9), ("multiword", 10), ("cluster2000_7_40", 11), ("cluster500_2_63", 12),
          ("cluster900_30_5", 13), ("dups1000", 14), ("dups65", 15)]


@pytest.fixture(scope="module")
def emu():
    return TM.load_tree_emu()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _leaves(keys, seed):
    return np.random.default_rng(seed).integers(0, 256, keys.shape, dtype=np.uint8)


def _partner(key, shared, rng):
    hx = key.tobytes().hex()
    other = "%x" % (int(hx[shared], 16) ^ (1 + int(rng.integers(0, 15))))
    tail = rng.integers(0, 256, 32, dtype=np.uint8).tobytes().hex()[shared + 1:]
    return np.frombuffer(bytes.fromhex(hx[:shared] + other + tail), np.uint8).copy()


# ---- 1. the model against itself ----
@pytest.mark.parametrize("name", TM.SEQUENCES)
def test_model_root_equals_the_bucket_recurrence(name):
    m, items = TM.Model(), 0
    for b in TM.sequence(name):
        root, c = m.apply(*b)
        assert TM.root_by_buckets(m.items) == root
        assert c[0] == len(m.items) == items + c[1] - c[3]
        items = c[0]
        assert c[1] + c[2] + c[3] + c[4] + c[5] == len(b[0])  # every row is exactly one of these
        assert c[7] == sum(1 for k in m.items if TM.bucket(k) in {TM.bucket(bytes(x)) for x in b[0]})


def test_model_semantics():
    rng = np.random.default_rng(20)
    k = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    lh = _leaves(k, 21)
    m = TM.Model()
    assert m.root() == SM.ZERO
    # the last row of a repeated key wins: set, delete, set with another leaf hash
    keys = np.stack([k[0], k[1], k[0], k[0]])
    root, c = m.apply(keys, np.stack([lh[0], lh[1], lh[2], lh[3]]), np.array([0, 0, 1, 0], np.uint8))
    assert m.items == {k[0].tobytes(): lh[3].tobytes(), k[1].tobytes(): lh[1].tobytes()}
    assert c == [2, 2, 0, 0, 0, 2, 2, 2]
    assert root == SM.model(k[:2], np.stack([lh[3], lh[1]]))[0]
    # ... and a delete as the last row: the earlier sets never happened
    root, c = m.apply(np.stack([k[2], k[2]]), None, np.array([0, 9], np.uint8))
    assert c == [2, 0, 0, 0, 1, 1, 1, 0] and len(m.items) == 2
    # no leaf hashes: the leaf is the key; a replace with the same value still counts as one
    root, c = m.apply(k[:1])
    assert c == [2, 0, 1, 0, 0, 0, 1, 1] and m.items[k[0].tobytes()] == k[0].tobytes()
    assert m.apply(k[:2], None, np.ones(2, np.uint8)) == (SM.ZERO, [0, 0, 0, 2, 0, 0, 2, 0])


@pytest.mark.parametrize("shared", [0, 3, 4, 5, 62, 63])
def test_recurrence_at_the_bucket_boundary(shared):
    rng = np.random.default_rng(30 + shared)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    b = _partner(a, shared, rng)
    assert SM.common_prefix(a.tobytes(), b.tobytes()) == shared
    m = TM.Model()
    one, _ = m.apply(a[None])
    two, _ = m.apply(b[None], _leaves(b[None], 31))
    assert TM.root_by_buckets(m.items) == two != one
    # a bucket of two keys has an inner node's hash, of one key the leaf hash
    cnt, h = TM.prefix_value(m.items, a.tobytes().hex()[:4])
    assert cnt == (2 if shared >= 4 else 1)
    assert (h == a.tobytes()) == (shared < 4)
    back, c = m.apply(b[None], None, np.ones(1, np.uint8))
    assert back == one and c[:5] == [1, 0, 0, 1, 0]


# ---- 2. the core against the model ----
def test_bucket_head_delta_and_positions(emu):
    rng = np.random.default_rng(40)
    for k in rng.integers(0, 256, (200, 32), dtype=np.uint8):
        assert emu.hostemu_tree_bucket(_p(k)) == TM.bucket(k.tobytes()) == int(k.tobytes().hex()[:4], 16)
    for edge in (bytes(32), b"\xff" * 32, b"\x00\x01" + bytes(30), b"\xff\xfe" + bytes(30)):
        k = np.frombuffer(edge, np.uint8)
        assert emu.hostemu_tree_bucket(_p(k)) == TM.bucket(edge)
    for last in (0, 1):
        for cp in range(65):
            assert emu.hostemu_tree_head(last, cp) == (1 if last or cp < 64 else 0)
    for d in (0, 1):
        for f in (0, 1):
            assert emu.hostemu_tree_delta(d, f) == TM.delta(d, f)
    for i, before in ((0, 0), (5, 3), (7, 0xFFFFFFFE), (1 << 24, 0xFFFFFF00)):  # a negative sum wraps
        assert emu.hostemu_tree_item_dest(i, before) == (i + before) & 0xFFFFFFFF
        assert emu.hostemu_tree_insert_dest(i, before) == (i + before) & 0xFFFFFFFF


def test_searches(emu):
    rng = np.random.default_rng(41)
    for shape, seed in (("random300", 1), ("cluster500_3_62", 2), ("dense", 3), ("random1", 4)):
        res = sorted({k.tobytes() for k in SM.case_keys(shape, seed)})
        m = len(res)
        sk = np.frombuffer(b"".join(res), np.uint8)
        probes = [res[int(i)] for i in rng.integers(0, m, 30)] + \
            [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(30)] + [bytes(32), b"\xff" * 32]
        if m > 1:
            probes += [_partner(np.frombuffer(res[m // 2], np.uint8), 63, rng).tobytes()]
        for pr in probes:
            found = ctypes.c_int(-1)
            pos = emu.hostemu_tree_lower_bound(_p(sk), m, _p(np.frombuffer(pr, np.uint8)), ctypes.byref(found))
            assert pos == sum(1 for r in res if r < pr) and found.value == (1 if pr in res else 0)
        assert emu.hostemu_tree_lower_bound(_p(sk), 0, _p(np.frombuffer(res[0], np.uint8)), ctypes.byref(found)) == 0
        assert found.value == 0
        for b in [0, 1, 0xFFFF, 0x10000] + [TM.bucket(r) + d for r in res[::17] for d in (0, 1)]:
            assert emu.hostemu_tree_bucket_begin(_p(sk), m, b) == sum(1 for r in res if TM.bucket(r) < b), b


def test_changes_before_an_item(emu):
    """From the changes' positions and found bits alone: how many changes have
    smaller keys than resident item i, and whether one has its key."""
    rng = np.random.default_rng(42)
    res = sorted({k.tobytes() for k in SM.case_keys("random60", 5)})
    for trial in range(20):
        ch = {res[int(i)] for i in rng.integers(0, len(res), 12)} | \
            {rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(int(rng.integers(0, 25)))}
        if trial == 0:
            ch = {bytes(32), b"\xff" * 32}
        ch = sorted(ch)
        pos = np.array([sum(1 for r in res if r < c) for c in ch], np.uint32)
        code = np.array([2 if c in res else 0 for c in ch], np.uint8)
        for i, r in enumerate(res):
            hit = ctypes.c_int(-1)
            got = emu.hostemu_tree_changes_before(_p(pos), _p(code), len(ch), i, ctypes.byref(hit))
            assert got == sum(1 for c in ch if c < r) and hit.value == (1 if r in ch else 0)
    hit = ctypes.c_int(-1)
    assert emu.hostemu_tree_changes_before(None, None, 0, 3, ctypes.byref(hit)) == 0 and hit.value == 0


def test_top_recurrence(emu):
    rng = np.random.default_rng(43)
    for trial in range(60):
        cnt = rng.integers(0, 4, 16).astype(np.uint32)
        if trial < 16:
            cnt[:] = 0
            cnt[trial] = 1 + trial % 2
        if trial == 16:
            cnt[:] = 0
        h = rng.integers(0, 256, (16, 32), dtype=np.uint8)
        for root in (0, 1):
            out = np.zeros(32, np.uint8)
            got = emu.hostemu_tree_top_value(_p(cnt), _p(h), root, _p(out))
            total = int(cnt.sum())
            assert got == total
            if total == 0:
                want = SM.ZERO
            elif total == 1 and not root:
                want = h[int(np.nonzero(cnt)[0][0])].tobytes()  # passed up unchanged
            else:  # a child without keys counts as empty whatever its hash bytes
                want = SM.inner_hash([h[c].tobytes() if cnt[c] else SM.ZERO for c in range(16)])
            assert out.tobytes() == want


# ---- 3. the staged apply ----
def _run(emu, cap, batches):
    m, e = TM.Model(), TM.EmuTree(emu, cap)
    try:
        for b in batches:
            want = m.apply(*b)
            rc, root, c = e.apply(*b)
            assert rc == 0 and c == want[1] and root == want[0]
            k, l = e.content()
            wk, wl = m.content()
            assert np.array_equal(k, wk) and np.array_equal(l, wl)
    finally:
        e.close()
    return m


@pytest.mark.parametrize("name", TM.SEQUENCES)
def test_the_staged_apply_equals_the_model(emu, name):
    _run(emu, 1200, TM.sequence(name))


@pytest.mark.parametrize("shape,seed", SHAPES)
def test_the_staged_apply_on_the_root_call_shapes(emu, shape, seed):
    """Loaded in one apply, the root is the root call's; then a mixed batch, then everything deleted."""
    keys = SM.case_keys(shape, seed)
    lh = _leaves(keys, seed + 100)
    rng = np.random.default_rng(seed)
    m = TM.Model()
    want, c = m.apply(keys, lh)
    assert c[0] == SM.model(keys)[1][0]
    mixed = TM._mixed_batch(rng, m.items, 1 + keys.shape[0] // 3)
    m = _run(emu, 2 * keys.shape[0] + 8, [(keys, lh, None), mixed])
    every, _ = m.content()
    e = TM.EmuTree(emu, keys.shape[0])
    assert e.apply(keys, lh)[1] == want
    # (the root call keeps the first of equal keys, the tree the last: equal only without repeats)
    if c[5] == 0:
        assert want == SM.model(keys, lh)[0]
    assert e.apply(keys, None, np.ones(keys.shape[0], np.uint8))[1] == SM.ZERO
    e.close()


def test_the_staged_apply_at_the_boundary_and_capacity(emu):
    rng = np.random.default_rng(50)
    batches = []
    for shared in (3, 4, 63):
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        b = _partner(a, shared, rng)
        batches += [(a[None], None, None), (b[None], _leaves(b[None], 51), None), (a[None], None, np.ones(1, np.uint8))]
    ends = np.stack([np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8)])
    batches += [(ends, None, None), (ends[:1], None, np.ones(1, np.uint8))]
    _run(emu, 16, batches)
    # the capacity: a batch is refused when the count after it would exceed it, and nothing changes
    e = TM.EmuTree(emu, 10)
    k = SM.case_keys("random12", 52)
    rc, root, c = e.apply(k[:6])
    assert rc == 0 and c[0] == 6
    assert e.apply(k[6:11])[0] == -1
    assert np.array_equal(e.content()[0], np.array(sorted(k[:6].tolist()), np.uint8))
    assert e.apply(np.zeros((0, 32), np.uint8))[1:] == (root, [6, 0, 0, 0, 0, 0, 0, 0])
    rc, _, c = e.apply(k[6:10])
    assert rc == 0 and c[:2] == [10, 4]
    e.close()


# ---- 4. the fixture ----
def test_golden_sequences(emu):
    with open(TM.GOLDEN) as f:
        doc = json.load(f)
    assert [s["name"] for s in doc["sequences"]] == TM.SEQUENCES and sum(len(s["steps"]) for s in doc["sequences"]) >= 18
    for s in doc["sequences"]:
        batches = TM.sequence(s["name"])
        assert len(batches) == len(s["steps"])
        m, e = TM.Model(), TM.EmuTree(emu, 1200)
        for b, want in zip(batches, s["steps"]):
            root, counts = m.apply(*b)
            assert (len(b[0]), root.hex(), counts) == (want["rows"], want["root"], want["counts"]), s["name"]
            rc, eroot, ecounts = e.apply(*b)
            assert (rc, eroot.hex(), ecounts) == (0, want["root"], want["counts"]), s["name"]
        e.close()


# ---- 5. the stand-alone sanitized program ----
def test_sanitized_program(tmp_path):
    """tests/native/shamap_tree_sanitize_main.cpp under ASan + UBSan, as a child
    process: the staged apply on exactly sized heap buffers over the shared
    sequences, a deep one-bucket tree, a tree filled to its capacity and a
    refused batch."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "shamap_tree_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("shamap_tree_sanitize_main.cpp", "hostemu_shamap_tree.cpp")]
    csrc = os.path.join(ROOT, "stellard_amd", "csrc")
    deps = srcs + [os.path.join(csrc, h) for h in ("stl_shamap_tree_core.h", "stl_shamap_core.h", "stl_sha512.h",
                                                   "stl_fe25519.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0]], check=True, cwd=ROOT)
    runs = [(1200, TM.sequence(n)) for n in TM.SEQUENCES]
    dense = SM.case_keys("dense", 60)
    runs.append((4096, [(dense[:3000], None, None),
                        (dense[2000:], _leaves(dense[2000:], 61), None),  # to the brim: 4,096 of 4,096
                        (dense[:1], None, None),                          # a replace on the full tree's bound
                        (dense[::2].copy(), None, np.ones(2048, np.uint8))]))
    k = SM.case_keys("random20", 62)
    runs.append((10, [(k[:6], None, None), (k[6:11], None, None), (k[6:10], None, None)]))  # the second is refused
    blob, steps = b"", 0
    for cap, batches in runs:
        m = TM.Model()
        blob += struct.pack("<II", cap, len(batches))
        for keys, lh, ops in batches:
            n = keys.shape[0]
            trial = TM.Model()
            trial.items = dict(m.items)
            refused = trial.apply(keys, lh, ops)[1][0] > cap  # the count afterwards decides, not the rows
            root, c = (m.root(), [0] * 8) if refused else m.apply(keys, lh, ops)
            blob += struct.pack("<IBB", n, lh is not None, ops is not None) + keys.tobytes()
            if lh is not None:
                blob += lh.tobytes()
            if ops is not None:
                blob += np.ascontiguousarray(ops, np.uint8).tobytes()
            wk, wl = m.content()
            blob += struct.pack("<i", -1 if refused else 0) + root + struct.pack("<8I", *c)
            blob += struct.pack("<I", wk.shape[0]) + wk.tobytes() + wl.tobytes()
            steps += 1
    data = tmp_path / "shamap_tree.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<I", len(runs)) + blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith(f"steps {steps} failed checks 0")
    assert "rc -1" in r.stdout and "items 4096" in r.stdout


# ---- 6. the C ABI without a GPU ----
def test_argument_checks():
    """Argument errors come before any device work, on every machine; a handle
    that is not live is STL_EINVAL whether or not there is a device."""
    import torch
    from stellard_amd import _native as N
    from stellard_amd import verify as V
    lib = N.load()
    buf = np.zeros(1024, np.uint8)
    base = (buf.ctypes.data + 127) & ~127
    p = lambda off=0: ctypes.c_void_p(base + off)  # noqa: E731
    fake = ctypes.c_void_p(base + 512)  # never a live tree
    h = ctypes.c_void_p()
    for cap in (0, N.STL_SHAMAP_MAX_ITEMS + 1, 0xFFFFFFFF):
        assert lib.stl_shamap_tree_create(cap, ctypes.byref(h)) == N.STL_EINVAL and not h.value
    assert lib.stl_shamap_tree_create(16, None) == N.STL_EINVAL
    dev, host = lib.stl_shamap_tree_apply_device, lib.stl_shamap_tree_apply
    # NULL tree, root, keys
    assert dev(None, p(), None, None, 1, p(64), None, None) == N.STL_EINVAL
    assert dev(fake, p(), None, None, 1, None, None, None) == N.STL_EINVAL
    assert dev(fake, None, None, None, 1, p(64), None, None) == N.STL_EINVAL
    assert host(None, p(), None, None, 1, p(64), None) == N.STL_EINVAL
    assert host(fake, p(), None, None, 1, None, None) == N.STL_EINVAL
    assert host(fake, None, None, None, 1, p(64), None) == N.STL_EINVAL
    for n in (N.STL_SHAMAP_MAX_ITEMS + 1, 1 << 32, (1 << 64) - 1):
        assert dev(fake, p(), None, None, n, p(64), None, None) == N.STL_EINVAL
        assert host(fake, p(), None, None, n, p(64), None) == N.STL_EINVAL
    # alignment: keys and leaf hashes 16, root and counts 4 (device form); ops any
    for off in (1, 4, 8):
        assert dev(fake, p(off), None, None, 1, p(64), None, None) == N.STL_EINVAL, off
        assert dev(fake, p(), p(128 + off), None, 1, p(64), None, None) == N.STL_EINVAL, off
    for off in (1, 2, 3):
        assert dev(fake, p(), None, None, 1, p(64 + off), None, None) == N.STL_EINVAL, off
        assert dev(fake, p(), None, None, 1, p(64), p(96 + off), None) == N.STL_EINVAL, off
        assert lib.stl_shamap_tree_root_device(fake, p(64 + off), None) == N.STL_EINVAL
        assert lib.stl_shamap_tree_export_device(fake, p(off), None, 4, None, None) == N.STL_EINVAL
        assert lib.stl_shamap_tree_export_device(fake, p(), None, 4, p(96 + off), None) == N.STL_EINVAL
    # well-formed calls on a handle that is not live
    assert dev(fake, p(), p(128), p(301), 2, p(64), p(96), None) == N.STL_EINVAL
    assert host(fake, p(1), p(129), p(257), 2, p(65), p(100)) == N.STL_EINVAL
    assert lib.stl_shamap_tree_root_device(fake, p(64), None) == N.STL_EINVAL
    assert lib.stl_shamap_tree_root_device(None, p(64), None) == N.STL_EINVAL
    assert lib.stl_shamap_tree_export_device(fake, p(), p(128), 4, p(96), None) == N.STL_EINVAL
    assert lib.stl_shamap_tree_export_device(fake, p(), None, N.STL_SHAMAP_MAX_ITEMS + 1, None, None) == N.STL_EINVAL
    info = V.ShamapTreeInfo(struct_size=ctypes.sizeof(V.ShamapTreeInfo))
    assert ctypes.sizeof(V.ShamapTreeInfo) == 64
    assert lib.stl_shamap_tree_get_info(fake, ctypes.byref(info)) == N.STL_EINVAL
    info.struct_size = 8
    assert lib.stl_shamap_tree_get_info(fake, ctypes.byref(info)) == N.STL_EINVAL
    assert lib.stl_shamap_tree_get_info(fake, None) == N.STL_EINVAL
    lib.stl_shamap_tree_destroy(None)
    lib.stl_shamap_tree_destroy(fake)  # ignored
    if not torch.cuda.is_available():
        assert lib.stl_shamap_tree_create(16, ctypes.byref(h)) == N.STL_ENODEV and not h.value
    assert not buf.any()  # nothing was written


def test_python_wrapper_refuses_wrong_dtypes_and_shapes():
    torch = pytest.importorskip("torch")
    from stellard_amd import verify as V
    tree = V.ShamapTree.__new__(V.ShamapTree)  # no handle: the checks come before the library is called
    tree._h = None
    n = 4
    t = lambda dt=torch.uint8, w=32, rows=n: torch.zeros((rows, w), dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="uint8"):
        tree.apply_device(t(torch.int32))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        tree.apply_device(t(w=20))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        tree.apply_device(torch.zeros(32 * n, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        tree.apply_device(t(), leaf_hashes=t(torch.int64, w=4))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        tree.apply_device(t(), leaf_hashes=t(rows=n - 1))
    with pytest.raises(ValueError, match=r"uint8\[n\]"):
        tree.apply_device(t(), ops=torch.zeros(n, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"uint8\[n\]"):
        tree.apply_device(t(), ops=torch.zeros(n + 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\(1, 32\)"):
        tree.apply_device(t(), out_root=torch.zeros(32, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"int32\[8\]"):
        tree.apply_device(t(), counts=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"int32\[8\]"):
        tree.apply_device(t(), counts=torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match="CUDA"):
        tree.apply_device(t())  # host tensors
    with pytest.raises(ValueError, match=r"\(1, 32\)"):
        tree.root_device(out_root=torch.zeros((2, 32), dtype=torch.uint8))
    with pytest.raises(ValueError, match="CUDA"):
        tree.root_device(out_root=torch.zeros((1, 32), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        tree.export_device(t(torch.int8))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        tree.export_device(t(), out_leaf_hashes=t(rows=n + 1))
    with pytest.raises(ValueError, match=r"int32\[1\]"):
        tree.export_device(t(), out_items=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="CUDA"):
        tree.export_device(t())
    # the host form
    k = np.zeros((n, 32), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        tree.apply(k.astype(np.int32))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        tree.apply(np.zeros((n, 20), np.uint8))
    with pytest.raises(ValueError, match="leaf_hashes"):
        tree.apply(k, leaf_hashes=np.zeros((n - 1, 32), np.uint8))
    with pytest.raises(ValueError, match="ops"):
        tree.apply(k, ops=np.zeros(n, np.int32))
    with pytest.raises(ValueError, match="ops"):
        tree.apply(k, ops=np.zeros(n + 1, np.uint8))
    if not torch.cuda.is_available():
        from stellard_amd import _native as N
        with pytest.raises(N.StlError) as e:
            V.ShamapTree(16)
        assert e.value.rc == N.STL_ENODEV
