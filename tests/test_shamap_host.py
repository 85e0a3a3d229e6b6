"""The SHAMap root on the host: the model of tests/shamap_py.py against itself
and against stellard_amd/csrc/stl_shamap_core.h compiled for the host by
tests/native/hostemu_shamap.cpp.

  * the model's two statements (recursive definition, insertion walk) agree on
    random, clustered, deep and duplicate-bearing sets, whatever the order,
  * the closed forms (neighbour bytes, node counts, depth histogram) agree
    with both,
  * the host emulation equals the model on the inner-node hash (also checked
    against hashlib directly), the nibble, the neighbour byte, the node rule,
    and on the whole root as the kernels stage it,
  * tests/golden/shamap_roots.json pins the model,
  * the same code in a stand-alone ASan + UBSan program (never loaded into Python),
  * the entry points' argument checks where there is no GPU, and the Python
    wrapper's dtype and shape checks."""
import ctypes
import hashlib
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import shamap_py as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SHAPES = [("random0", 1), ("random1", 2), ("random2", 3), ("random17", 4), ("random300", 5), ("random5000", 6),
          ("root17", 7), ("deepest", 8), ("dense", 9), ("multiword", 10), ("cluster2000_7_40", 11),
          ("cluster500_2_63", 12), ("cluster900_30_5", 13), ("dups1000", 14), ("dups65", 15)]


@pytest.fixture(scope="module")
def emu():
    return SM.load_shamap_emu()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _leaves(keys, seed):
    return np.random.default_rng(seed).integers(0, 256, keys.shape, dtype=np.uint8)


# ---- 1. the model against itself ----
@pytest.mark.parametrize("shape,seed", SHAPES)
def test_the_two_models_agree(shape, seed):
    keys = SM.case_keys(shape, seed)
    leaves = _leaves(keys, seed + 100)
    for lh in (None, leaves):
        items, nsel = SM.the_set(keys, lh)
        root, nodes, deep = SM.root_recursive(items)
        rows = [(k.tobytes(), (k if lh is None else lh[i]).tobytes()) for i, k in enumerate(keys)]
        assert SM.root_by_insertion(rows) == (root, nodes, deep, nsel - len(items))
        assert SM.counts(keys) == [len(items), nsel - len(items), nodes, deep]
        if len(items) == 0:
            assert root == SM.ZERO and nodes == 0
        # insertion order does not show in the root: the distinct items backwards and shuffled
        distinct = list(items.items())
        rng = np.random.default_rng(seed)
        for order in (distinct[::-1], [distinct[i] for i in rng.permutation(len(distinct))]):
            assert SM.root_by_insertion(order) == (root, nodes, deep, 0)


def test_shapes_the_contract_names():
    """One item: its leaf sits under the root.  Two keys that part at the last
    nibble: 64 inner nodes, the deepest at depth 63.  The worst case of n keys
    is 63 (n - 1) + 1 inner nodes."""
    k = SM.case_keys("random1", 1)
    root, c = SM.model(k)
    assert c == [1, 0, 1, 0]
    b = k[0, 0] >> 4
    assert root == SM.inner_hash([k[0].tobytes() if i == b else SM.ZERO for i in range(16)])
    assert SM.model(SM.case_keys("deepest", 2))[1] == [2, 0, 64, 63]
    # five keys in one depth-63 node: still one chain of 64
    chain = np.zeros((5, 32), np.uint8)
    chain[:, 31] = np.arange(5)
    assert SM.model(chain)[1] == [5, 0, 64, 63]
    # n keys in pairs that part at the last nibble, the pairs parting at the root: 63 * n / 2 + 1 nodes
    pairs = np.zeros((8, 32), np.uint8)
    pairs[:, 0] = np.arange(8) // 2 << 4
    pairs[:, 31] = np.arange(8) % 2
    assert SM.model(pairs)[1] == [8, 0, 63 * 4 + 1, 63]
    assert SM.model(np.zeros((0, 32), np.uint8)) == (SM.ZERO, [0, 0, 0, 0])


def test_select_and_leaf_hashes_in_the_model():
    keys = SM.case_keys("dups1000", 3)
    leaves = _leaves(keys, 4)
    sel = np.random.default_rng(5).random(keys.shape[0]) < 0.5
    root, c = SM.model(keys, leaves, sel)
    sub = np.nonzero(sel)[0]
    assert (root, c) == SM.model(keys[sub], leaves[sub])
    assert c[0] + c[1] == int(sel.sum())
    # of equal keys the lowest selected row's leaf hash counts
    k2 = np.concatenate([keys[:3], keys[:3]])
    l2 = _leaves(k2, 6)
    assert SM.model(k2, l2)[0] == SM.model(keys[:3], l2[:3])[0] != SM.model(keys[:3], l2[3:])[0]
    assert SM.model(k2, l2, [False, True, True, True, True, True])[0] == \
        SM.model(keys[:3], np.concatenate([l2[3:4], l2[1:3]]))[0]


# ---- 2. the core against the model ----
def test_inner_hash(emu):
    rng = np.random.default_rng(21)
    for trial in range(64):
        slots = rng.integers(0, 256, (16, 32), dtype=np.uint8)
        if trial == 0:
            slots[:] = 0
        elif trial == 1:
            slots[:] = 0xFF
        elif trial % 3 == 0:
            slots[rng.random(16) < 0.6] = 0  # empty branches
        out = np.zeros(32, np.uint8)
        emu.hostemu_shamap_inner_hash(_p(slots), _p(out))
        assert out.tobytes() == hashlib.sha512(b"MIN\0" + slots.tobytes()).digest()[:32]
        assert out.tobytes() == SM.inner_hash([s.tobytes() for s in slots])


def test_nibble_prefix_order_and_sort_words(emu):
    rng = np.random.default_rng(22)
    keys = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    for k in keys[:40]:
        for d in range(64):
            assert emu.hostemu_shamap_nibble(_p(k), d) == SM.nibble(k.tobytes(), d) == int(k.tobytes().hex()[d], 16)
        assert [emu.hostemu_shamap_sort_word(_p(k), w) for w in range(4)] == \
            [int.from_bytes(k.tobytes()[8 * w: 8 * w + 8], "big") for w in range(4)]
    for i in range(199):
        a = keys[i]
        for cut in (None, 0, 1, 7, 8, 16, 31, 63, 64):
            b = keys[i + 1].copy()
            if cut is not None:  # b shares exactly `cut` nibbles with a (or is a)
                hx = a.tobytes().hex()
                if cut < 64:
                    other = "%x" % (int(hx[cut], 16) ^ (1 + i % 15))
                    hx = hx[:cut] + other + b.tobytes().hex()[cut + 1:]
                b = np.frombuffer(bytes.fromhex(hx), np.uint8).copy()
            cp = emu.hostemu_shamap_common_prefix(_p(a), _p(b))
            assert cp == SM.common_prefix(a.tobytes(), b.tobytes())
            if cut is not None:
                assert cp == cut
            assert emu.hostemu_shamap_key_less(_p(a), _p(b)) == (a.tobytes() < b.tobytes())
            assert emu.hostemu_shamap_key_less(_p(b), _p(a)) == (b.tobytes() < a.tobytes())


def test_neighbour_byte_and_node_rule(emu):
    for shape, seed in SHAPES:
        keys = sorted({k.tobytes() for k in SM.case_keys(shape, seed)})
        want = SM.neighbours(keys) if keys else []
        m = len(keys)
        got = []
        for i, k in enumerate(keys):
            a = np.frombuffer(k, np.uint8)
            nxt = np.frombuffer(keys[i + 1], np.uint8) if i + 1 < m else None
            got.append(emu.hostemu_shamap_neighbour(_p(a), _p(nxt) if nxt is not None else None, i + 1 == m, m == 1))
        assert got == want
    for lp in range(-1, 64):
        for lc in range(-1, 64):
            assert emu.hostemu_shamap_leaf_parent_depth(lp, lc) == max(lp, lc, 0)
            for d in range(64):
                assert emu.hostemu_shamap_starts_node(lp, lc, d) == (1 if lp < d <= lc else 0)


def test_range_and_branch_search(emu):
    keys = sorted({k.tobytes() for k in SM.case_keys("cluster900_30_5", 31)})
    m = len(keys)
    sk = np.frombuffer(b"".join(keys), np.uint8)
    l = SM.neighbours(keys)
    for a in range(0, m, 7):
        for d in range(0, 8):
            if not (d == 0 or SM.common_prefix(keys[a], keys[min(a + 1, m - 1)]) >= d):
                continue
            e = next((i for i in range(a + 1, m) if SM.common_prefix(keys[a], keys[i]) < d), m)
            assert emu.hostemu_shamap_range_end(_p(sk), m, a, d) == e
            for c in range(16):
                first = next((i for i in range(a, e) if SM.nibble(keys[i], d) == c), e)
                assert emu.hostemu_shamap_branch_first(_p(sk), a, e, d, c) == first
    assert len(l) == m


@pytest.mark.parametrize("shape,seed", SHAPES)
def test_the_staged_computation_equals_the_model(emu, shape, seed):
    keys = SM.case_keys(shape, seed)
    n = keys.shape[0]
    leaves = _leaves(keys, seed + 200)
    sel = np.random.default_rng(seed + 300).random(n) < 0.6
    for lh, s in ((None, None), (leaves, None), (None, sel), (leaves, sel),
                  (leaves, np.zeros(n, bool)), (None, np.ones(n, bool))):
        root, c = SM.model(keys, lh, s)
        got_root, got_c, hist, l = SM.emu_root(emu, keys, lh, s)
        assert (got_root, got_c) == (root, c)
        srt = sorted(SM.the_set(keys, lh, s)[0])
        assert hist == SM.depth_histogram(srt)
        assert l == (SM.neighbours(srt) if srt else [])


# ---- 3. the fixture ----
def test_golden_roots():
    with open(SM.GOLDEN) as f:
        doc = json.load(f)
    assert [(c["shape"], c["seed"]) for c in doc["cases"]] == SM.GOLDEN_CASES and len(doc["cases"]) >= 12
    for c in doc["cases"]:
        keys = SM.case_keys(c["shape"], c["seed"])
        assert keys.shape[0] == c["n"]
        root, counts = SM.model(keys)
        assert (root.hex(), counts) == (c["root"], c["counts"]), c["shape"]


# ---- 4. the stand-alone sanitized program ----
def test_sanitized_program(tmp_path):
    """tests/native/shamap_sanitize_main.cpp under ASan + UBSan, as a child
    process: the staged computation on exactly sized heap buffers over the
    shapes above, with and without leaf hashes and a select bitmap."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "shamap_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("shamap_sanitize_main.cpp", "hostemu_shamap.cpp")]
    csrc = os.path.join(ROOT, "stellard_amd", "csrc")
    deps = srcs + [os.path.join(csrc, h) for h in ("stl_shamap_core.h", "stl_sha512.h", "stl_fe25519.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0]], check=True, cwd=ROOT)
    blob = b""
    cases = 0
    for shape, seed in SHAPES:
        keys = SM.case_keys(shape, seed)
        n = keys.shape[0]
        leaves = _leaves(keys, seed + 200)
        sel = np.random.default_rng(seed + 300).random(n) < 0.6
        for lh, s in ((None, None), (leaves, sel)):
            root, c = SM.model(keys, lh, s)
            blob += struct.pack("<IBB", n, lh is not None, s is not None) + keys.tobytes()
            if lh is not None:
                blob += lh.tobytes()
            if s is not None:
                blob += np.packbits(s, bitorder="little").tobytes()
            blob += root + struct.pack("<4I", *c)
            cases += 1
    data = tmp_path / "shamap.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<I", cases) + blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith(f"cases {cases} failed checks 0")
    assert "deepest 63" in r.stdout


# ---- 5. the C ABI without a GPU ----
def test_argument_checks():
    """Argument errors come before any device work, on every machine; without
    a device every well-formed call is STL_ENODEV."""
    import torch
    from stellard_amd import _native as N
    lib = N.load()
    assert N.STL_SHAMAP_MAX_ITEMS == SM.MAX_ITEMS == 1 << 24
    buf = np.zeros(1024, np.uint8)
    base = (buf.ctypes.data + 127) & ~127
    p = lambda off=0: ctypes.c_void_p(base + off)  # noqa: E731
    dev, host = lib.stl_shamap_root_device, lib.stl_shamap_root
    # NULL root; NULL keys with rows
    assert dev(p(), None, None, 1, None, None, None) == N.STL_EINVAL
    assert dev(None, None, None, 1, p(64), None, None) == N.STL_EINVAL
    assert host(p(), None, None, 1, None, None) == N.STL_EINVAL
    assert host(None, None, None, 1, p(64), None) == N.STL_EINVAL
    # the row limit
    for n in (N.STL_SHAMAP_MAX_ITEMS + 1, 1 << 32, (1 << 64) - 1):
        assert dev(p(), None, None, n, p(64), None, None) == N.STL_EINVAL
        assert host(p(), None, None, n, p(64), None) == N.STL_EINVAL
    # alignment: keys and leaf hashes 16, root and counts 4 (device form)
    for off in (1, 4, 8):
        assert dev(p(off), None, None, 1, p(64), None, None) == N.STL_EINVAL, off
        assert dev(p(), p(128 + off), None, 1, p(64), None, None) == N.STL_EINVAL, off
    for off in (1, 2, 3):
        assert dev(p(), None, None, 1, p(64 + off), None, None) == N.STL_EINVAL, off
        assert dev(p(), None, None, 1, p(64), p(96 + off), None) == N.STL_EINVAL, off
    if not torch.cuda.is_available():
        assert dev(p(), None, None, 1, p(64), None, None) == N.STL_ENODEV
        assert dev(p(), p(128), p(256), 2, p(64), p(96), None) == N.STL_ENODEV
        assert dev(None, None, None, 0, p(64), None, None) == N.STL_ENODEV
        assert dev(p(), None, None, N.STL_SHAMAP_MAX_ITEMS, p(64), None, None) == N.STL_ENODEV
        assert host(p(), None, None, 1, p(64), None) == N.STL_ENODEV
        assert host(p(1), p(129), p(257), 2, p(65), p(100)) == N.STL_ENODEV  # host arrays: any alignment
        assert not buf.any()  # nothing was written


def test_python_wrapper_refuses_wrong_dtypes_and_shapes():
    torch = pytest.importorskip("torch")
    from stellard_amd import verify as V
    assert V.SHAMAP_MAX_ITEMS == 1 << 24
    n = 4
    t = lambda dt=torch.uint8, w=32, rows=n: torch.zeros((rows, w), dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="uint8"):
        V.shamap_root_device(t(torch.int32))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        V.shamap_root_device(t(w=20))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        V.shamap_root_device(torch.zeros(32 * n, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        V.shamap_root_device(t(), leaf_hashes=t(torch.int64, w=4))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        V.shamap_root_device(t(), leaf_hashes=t(rows=n - 1))
    with pytest.raises(ValueError, match="int64"):
        V.shamap_root_device(t(), select_words=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        V.shamap_root_device(t(rows=65), select_words=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\(1, 32\)"):
        V.shamap_root_device(t(), out_root=torch.zeros(32, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        V.shamap_root_device(t(), out_root=torch.zeros((1, 32), dtype=torch.int8))
    with pytest.raises(ValueError, match=r"int32\[4\]"):
        V.shamap_root_device(t(), counts=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"int32\[4\]"):
        V.shamap_root_device(t(), counts=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="CUDA"):
        V.shamap_root_device(t())  # host tensors
    # the host form
    k = np.zeros((n, 32), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        V.shamap_root(k.astype(np.int32))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        V.shamap_root(np.zeros((n, 20), np.uint8))
    with pytest.raises(ValueError, match="leaf_hashes"):
        V.shamap_root(k, leaf_hashes=np.zeros((n - 1, 32), np.uint8))
    with pytest.raises(ValueError, match="bool"):
        V.shamap_root(k, select=np.ones(n, np.uint8))
    with pytest.raises(ValueError, match="bool"):
        V.shamap_root(k, select=np.ones(n + 1, bool))
    if not torch.cuda.is_available():
        from stellard_amd import _native as N
        with pytest.raises(N.StlError) as e:
            V.shamap_root(k)
        assert e.value.rc == N.STL_ENODEV
