"""The stored inner nodes of a SHAMap on the host: the model of
tests/shamap_nodes_py.py against itself and against the shared device code
(stl_shamap_core.h, stl_shamap_tree_core.h) compiled for the host by
tests/native/hostemu_shamap_nodes.cpp.

  * the model's two statements (insertion tree, closed form) give the same dict,
  * every body hashes (hashlib) to its hash, the root node's hash is
    shamap_py.model's root and the dict's size is counts[2],
  * the host emulation equals the model on the masking, leaf, meta and
    top-emission rules and on both staged computations, overflow included,
  * nodes(new) - nodes(old) <= E <= nodes(new) (by hash on the left) on random
    and on bucket-boundary batches,
  * the same code in a stand-alone ASan + UBSan program (never loaded into Python),
  * the entry points' argument checks, which need no device,
  * tests/golden/shamap_nodes.json pins the model."""
import ctypes
import hashlib
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import shamap_nodes_py as NM
from tests import shamap_py as SM
from tests import shamap_tree_py as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SHAPES = [("random0", 1), ("random1", 2), ("random2", 3), ("random3", 16), ("random17", 4), ("random300", 5),
          ("random3000", 6), ("root17", 7), ("deepest", 8), ("dense", 9), ("multiword", 10), ("cluster2000_7_40", 11),
          ("cluster500_2_63", 12), ("cluster900_30_5", 13), ("dups1000", 14), ("dups65", 15)]


@pytest.fixture(scope="module")
def emu():
    return NM.load_nodes_emu()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _leaves(keys, seed):
    return np.random.default_rng(seed).integers(0, 256, np.asarray(keys).shape, dtype=np.uint8)


def _partner(key, shared, rng):
    """A key that shares exactly `shared` nibbles with key."""
    hx = bytes(key).hex()
    other = "%x" % (int(hx[shared], 16) ^ (1 + int(rng.integers(0, 15))))
    tail = rng.integers(0, 256, 32, dtype=np.uint8).tobytes().hex()[shared + 1:]
    return np.frombuffer(bytes.fromhex(hx[:shared] + other + tail), np.uint8).copy()


# ---- 1. the model against itself ----
@pytest.mark.parametrize("shape,seed", SHAPES)
def test_the_two_statements_agree(shape, seed):
    keys = SM.case_keys(shape, seed)
    for lh in (None, _leaves(keys, seed + 100)):
        items, _ = SM.the_set(keys, lh)
        closed = NM.nodes_closed(items)
        assert closed == NM.nodes_by_insertion(items)
        root, counts = SM.model(keys, lh)
        assert len(closed) == counts[2]
        assert max((d for d, _ in closed), default=0) == counts[3]
        for (d, nid), (h, body, mask) in closed.items():
            assert len(body) == 512 and hashlib.sha512(b"MIN\0" + body).digest()[:32] == h
            assert NM.masked(nid, d) == nid
            if len(items) > 300:
                continue  # the definition, branch by branch, on the small sets
            for c in range(16):
                child = body[32 * c: 32 * c + 32]
                under = [k for k in items if NM.masked(k, d) == nid and SM.nibble(k, d) == c]
                assert bool(mask >> c & 1) == (len(under) == 1)
                if not under:
                    assert child == SM.ZERO
                elif len(under) == 1:
                    assert child == items[under[0]]
                elif len(under) > 1:
                    assert child == closed[(d + 1, NM.masked(under[0], d + 1))][0]
        if items:
            assert closed[(0, SM.ZERO)][0] == root
        else:
            assert closed == {} and root == SM.ZERO


def test_shapes_the_contract_names():
    """One key: the root alone, its one branch a leaf.  Two keys that part at
    nibble 63: a chain of 64 nodes, only the deepest with leaves."""
    k = SM.case_keys("random1", 1)
    n = NM.nodes(k)
    assert list(n) == [(0, SM.ZERO)] and n[(0, SM.ZERO)][2] == 1 << (int(k[0, 0]) >> 4)
    deep = SM.case_keys("deepest", 2)
    n = NM.nodes(deep)
    assert sorted(d for d, _ in n) == list(range(64))
    for (d, nid), (_, _, mask) in n.items():
        assert nid == NM.masked(deep[0], d)
        assert mask == ((1 << 3 | 1 << 12) if d == 63 else 0)
    # the bound: m keys in pairs that part at the last nibble make 63 m / 2 + 1 nodes
    pairs = np.zeros((8, 32), np.uint8)
    pairs[:, 0] = np.arange(8) // 2 << 4
    pairs[:, 31] = np.arange(8) % 2
    assert len(NM.nodes(pairs)) == 63 * 4 + 1 <= 63 * (8 - 1) + 1


# ---- 2. the core's rules ----
def test_mask_leaf_and_meta_rules(emu):
    rng = np.random.default_rng(21)
    for k in rng.integers(0, 256, (20, 32), dtype=np.uint8):
        for d in range(64):
            out = np.zeros(32, np.uint8)
            emu.hostemu_nodes_mask_key(_p(k), d, _p(out))
            assert out.tobytes() == NM.masked(k, d) == bytes.fromhex(k.tobytes().hex()[:d] + "0" * (64 - d))
    ones = np.full(32, 0xFF, np.uint8)
    out = np.zeros(32, np.uint8)
    emu.hostemu_nodes_mask_key(_p(ones), 64, _p(out))  # never asked for, still the whole key
    assert out.tobytes() == ones.tobytes()
    l = np.array([5, 3, 7, 7, -1], np.int8)
    for p in range(5):
        for e in range(p + 1, 6):
            for d in range(0, 10):
                assert emu.hostemu_nodes_branch_is_leaf(_p(l), p, e, d) == (1 if p + 1 == e or l[p] <= d else 0)
    for d in (0, 1, 63):
        for mask in (0, 1, 0x8001, 0xFFFF):
            assert emu.hostemu_nodes_meta(d, mask) == NM.meta_word(d, mask) == d | mask << 16


def test_top_rules(emu):
    for cnt in range(4):
        for root in (0, 1):
            for dirty in (0, 1):
                want = bool(dirty) and (cnt >= 2 or (bool(root) and cnt >= 1))
                assert emu.hostemu_nodes_top_emits(cnt, root, dirty) == int(want)
    rng = np.random.default_rng(22)
    for depth, t in ((3, 0xABC), (3, 0), (3, 0xFFF), (2, 0x5E), (1, 0xD), (0, 0)):
        cnt = rng.integers(0, 4, 16).astype(np.uint32)
        h = rng.integers(0, 256, (16, 32), dtype=np.uint8)
        body, nid = np.zeros(512, np.uint8), np.zeros(32, np.uint8)
        leaf = emu.hostemu_nodes_top_node(_p(cnt), _p(h), depth, t, _p(body), _p(nid))
        assert leaf == sum(1 << c for c in range(16) if cnt[c] == 1)
        assert body.tobytes() == b"".join(h[c].tobytes() if cnt[c] else SM.ZERO for c in range(16))
        assert nid.tobytes() == bytes.fromhex(("%0*x" % (depth, t) if depth else "") + "0" * (64 - depth))


# ---- 3. the staged set computation ----
@pytest.mark.parametrize("shape,seed", SHAPES)
def test_the_staged_set_equals_the_model(emu, shape, seed):
    keys = SM.case_keys(shape, seed)
    n = keys.shape[0]
    leaves = _leaves(keys, seed + 200)
    sel = np.random.default_rng(seed + 300).random(n) < 0.6
    for lh, s in ((None, None), (leaves, None), (leaves, sel), (None, np.zeros(n, bool))):
        want = NM.nodes(keys, lh, s)
        root, counts, out = NM.emu_set(emu, keys, lh, s)
        assert (root, counts) == SM.model(keys, lh, s)
        assert int(out.count[0]) == counts[2] == len(want)
        assert out.as_dict() == want and out.guards_intact()


def test_the_staged_set_overflows_within_bounds(emu):
    keys = SM.case_keys("cluster900_30_5", 31)
    want = NM.nodes(keys)
    full = len(want)
    for max_nodes in (0, 1, 127, 128, 129, full - 1, full):
        root, counts, out = NM.emu_set(emu, keys, max_nodes=max_nodes)
        assert (root, counts) == SM.model(keys) and int(out.count[0]) == full
        got = out.as_dict()
        assert len(got) == min(max_nodes, full) and all(want[k] == v for k, v in got.items())
        assert out.guards_intact()
    # id and meta left out: hash and body alone
    _, _, out = NM.emu_set(emu, keys, ids=False, meta=False)
    assert {(out.hash[j].tobytes(), out.body[j].tobytes()) for j in range(full)} == \
        {(v[0], v[1]) for v in want.values()}


# ---- 4. what an apply stores ----
def _batches(name):
    """Seeded (old items, batch) pairs: random and bucket-boundary ones."""
    rng = np.random.default_rng({"random": 141, "boundary": 142, "collapse": 143, "absent": 144, "one_bucket": 145}[name])
    m = TM.Model()
    if name == "random":
        k = SM.case_keys("random2000", 41)
        m.apply(k, _leaves(k, 46))
        return m, [TM._mixed_batch(rng, m.items, rows) for rows in (1, 40, 300)]
    if name == "boundary":
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        ks = [a] + [_partner(a, s, rng) for s in (0, 1, 2, 3, 4, 5, 63)]
        k = np.stack(ks)
        m.apply(k[:4], _leaves(k[:4], 47))
        return m, [(k[4:5], None, None), (k[5:], _leaves(k[5:], 48), None), (k[3:6], None, np.ones(3, np.uint8)),
                   (k[:1], _leaves(k[:1], 49), None)]
    if name == "collapse":
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        b = _partner(a, 9, rng)
        c = _partner(a, 2, rng)
        k = np.stack([a, b, c])
        m.apply(k)
        dele = np.ones(1, np.uint8)
        return m, [(k[1:2], None, dele), (k[0:1], None, dele), (k[2:3], None, dele), (k, None, None)]
    if name == "absent":
        k = SM.case_keys("random500", 44)
        m.apply(k)
        gone = rng.integers(0, 256, (30, 32), dtype=np.uint8)
        return m, [(gone, None, np.ones(30, np.uint8))]
    k = np.unique(SM.case_keys("cluster400_1_50", 45), axis=0)
    m.apply(k[:300], _leaves(k[:300], 50))
    return m, [(k[300:], None, None), (k[:50], None, np.ones(50, np.uint8))]


@pytest.mark.parametrize("name", ["random", "boundary", "collapse", "absent", "one_bucket"])
def test_what_an_apply_stores(emu, name):
    """nodes(new) - nodes(old) <= E <= nodes(new), the staged apply stores E
    exactly, and its root and content are the model's."""
    m, batches = _batches(name)
    for batch in batches:
        old_items = dict(m.items)
        old = NM.nodes_closed(old_items)
        root, counts = m.apply(*batch)
        new = NM.nodes_closed(m.items)
        e = NM.emitted(m.items, batch[0], new)
        assert all(new[k] == v for k, v in e.items())
        old_hashes = NM.hashes_of(old)
        fresh = {k for k, v in new.items() if v[0] not in old_hashes}
        assert fresh <= set(e), "a node with a new hash is not stored"
        if name == "absent":
            assert not fresh and counts[6] > 0 and e  # nothing changed, the dirty buckets' nodes are stored all the same
        got_root, ndirty, gathered, nk, nl, out = NM.emu_apply(emu, old_items, *batch)
        assert (got_root, ndirty, gathered) == (root, counts[6], counts[7])
        wk, wl = m.content()
        assert np.array_equal(nk, wk) and np.array_equal(nl, wl)
        assert int(out.count[0]) == len(e) and out.as_dict() == e and out.guards_intact()
        for max_nodes in (0, 1, max(len(e) - 1, 0)):
            _, _, _, _, _, small = NM.emu_apply(emu, old_items, *batch, max_nodes=max_nodes)
            got = small.as_dict()
            assert int(small.count[0]) == len(e) and len(got) == min(max_nodes, len(e))
            assert all(e[k] == v for k, v in got.items()) and small.guards_intact()


# ---- 5. the fixture ----
def test_golden_nodes():
    with open(NM.GOLDEN) as f:
        doc = json.load(f)
    assert doc == NM.golden_document()
    assert sum(len(s["nodes"]) for s in doc["sets"]) >= 64 and doc["apply"]["stored"]


# ---- 6. the stand-alone sanitized program ----
def test_sanitized_program(tmp_path):
    """tests/native/shamap_nodes_sanitize_main.cpp under ASan + UBSan, as a
    child process: both staged computations with exactly sized output arrays,
    with room for every node and with too little."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "shamap_nodes_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("shamap_nodes_sanitize_main.cpp", "hostemu_shamap_nodes.cpp")]
    csrc = os.path.join(ROOT, "stellard_amd", "csrc")
    deps = srcs + [os.path.join(csrc, h) for h in ("stl_shamap_tree_core.h", "stl_shamap_core.h", "stl_sha512.h",
                                                   "stl_fe25519.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0]], check=True, cwd=ROOT)
    blob, cases = b"", 0
    for shape, seed in SHAPES:
        keys = SM.case_keys(shape, seed)
        n = keys.shape[0]
        leaves = _leaves(keys, seed + 200)
        sel = np.random.default_rng(seed + 300).random(n) < 0.6
        for lh, s in ((None, None), (leaves, sel)):
            root, c = SM.model(keys, lh, s)
            for max_nodes in sorted({c[2], c[2] // 2, 0}):
                blob += struct.pack("<BII", 0, max_nodes, n) + struct.pack("<BB", lh is not None, s is not None)
                blob += keys.tobytes() + (lh.tobytes() if lh is not None else b"")
                blob += np.packbits(s, bitorder="little").tobytes() if s is not None else b""
                blob += root + struct.pack("<I", c[2])
                cases += 1
    for name in ("random", "boundary", "collapse", "absent", "one_bucket"):
        m, batches = _batches(name)
        for keys, lh, ops in batches:
            ok, ol = m.content()
            root, _ = m.apply(keys, lh, ops)
            count = len(NM.emitted(m.items, keys))
            for max_nodes in sorted({count, count // 2}):
                blob += struct.pack("<BII", 1, max_nodes, ok.shape[0]) + ok.tobytes() + ol.tobytes()
                blob += struct.pack("<IBB", keys.shape[0], lh is not None, ops is not None) + keys.tobytes()
                blob += (lh.tobytes() if lh is not None else b"") + (ops.tobytes() if ops is not None else b"")
                blob += root + struct.pack("<I", count)
                cases += 1
    data = tmp_path / "shamap_nodes.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<I", cases) + blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"cases {cases} rows " in r.stdout and r.stdout.strip().endswith("failed checks 0")


# ---- 7. the C ABI without a GPU ----
def test_argument_checks():
    """A NULL out, hash, body or count, a wrong struct_size, too many rows and
    (device form) a misaligned array are STL_EINVAL before any device work;
    without a device every well-formed call is STL_ENODEV."""
    import torch
    from stellard_amd import _native as N
    lib = N.load()
    assert N.STL_SHAMAP_MAX_NODES == NM.MAX_NODES == 0xFFFFFFC0 and N.STL_SHAMAP_NODE_BODY_BYTES == 512
    assert ctypes.sizeof(N.ShamapNodesOut) == 48
    buf = np.zeros(4096, np.uint8)
    base = (buf.ctypes.data + 127) & ~127
    p = lambda off=0: ctypes.c_void_p(base + off)  # noqa: E731

    def out(**kw):
        f = dict(struct_size=ctypes.sizeof(N.ShamapNodesOut), max_nodes=2, hash=base + 256, body=base + 512,
                 id=base + 2048, meta=base + 2304, count=base + 2432)
        f.update(kw)
        return ctypes.byref(N.ShamapNodesOut(f["struct_size"], f["max_nodes"], f["hash"], f["body"], f["id"], f["meta"],
                                             f["count"]))

    tree = ctypes.c_void_p(base + 3000)  # never a live handle: well-formed calls on it are STL_EINVAL too
    calls = [
        ("set device", True, lambda o: lib.stl_shamap_nodes_device(p(), None, None, 1, p(64), p(96), o, None)),
        ("set host", False, lambda o: lib.stl_shamap_nodes(p(), None, None, 1, p(64), p(96), o)),
        ("apply device", True,
         lambda o: lib.stl_shamap_tree_apply_nodes_device(tree, p(), None, None, 1, p(64), p(96), o, None)),
        ("apply host", False, lambda o: lib.stl_shamap_tree_apply_nodes(tree, p(), None, None, 1, p(64), p(96), o)),
    ]
    for name, device_form, call in calls:
        assert call(None) == N.STL_EINVAL, name
        for bad in (dict(hash=None), dict(body=None), dict(count=None), dict(struct_size=40), dict(struct_size=0),
                    dict(struct_size=56), dict(max_nodes=0xFFFFFFC1), dict(max_nodes=0xFFFFFFFF)):
            assert call(out(**bad)) == N.STL_EINVAL, (name, bad)
        if device_form:
            for field in ("hash", "body", "id"):
                for off in (1, 4, 8):
                    assert call(out(**{field: base + 512 + off})) == N.STL_EINVAL, (name, field, off)
            for field in ("meta", "count"):
                for off in (1, 2, 3):
                    assert call(out(**{field: base + 2304 + off})) == N.STL_EINVAL, (name, field, off)
    # what the calls they extend refuse is refused still
    assert lib.stl_shamap_nodes_device(p(), None, None, 1, None, None, out(), None) == N.STL_EINVAL
    assert lib.stl_shamap_nodes_device(p(1), None, None, 1, p(64), None, out(), None) == N.STL_EINVAL
    assert lib.stl_shamap_nodes(None, None, None, 1, p(64), None, out()) == N.STL_EINVAL
    assert lib.stl_shamap_nodes_device(p(), None, None, N.STL_SHAMAP_MAX_ITEMS + 1, p(64), None, out(), None) == \
        N.STL_EINVAL
    assert lib.stl_shamap_tree_apply_nodes_device(None, p(), None, None, 1, p(64), None, out(), None) == N.STL_EINVAL
    assert lib.stl_shamap_tree_apply_nodes(None, p(), None, None, 1, p(64), None, out()) == N.STL_EINVAL
    if not torch.cuda.is_available():
        ok = out(id=None, meta=None, max_nodes=0)
        assert lib.stl_shamap_nodes_device(p(), None, None, 1, p(64), None, ok, None) == N.STL_ENODEV
        assert lib.stl_shamap_nodes_device(None, None, None, 0, p(64), None, out(), None) == N.STL_ENODEV
        assert lib.stl_shamap_nodes(p(1), p(129), None, 2, p(65), p(100),
                                    out(hash=base + 257, body=base + 513, id=base + 2049, meta=base + 2305,
                                        count=base + 2433)) == N.STL_ENODEV  # host arrays: any alignment
        assert lib.stl_shamap_nodes(p(), None, None, 1, p(64), None, out(max_nodes=0xFFFFFFC0)) == N.STL_ENODEV
        assert not buf.any()  # nothing was written


def test_python_wrapper_refuses_wrong_arguments():
    torch = pytest.importorskip("torch")
    from stellard_amd import verify as V
    assert V.SHAMAP_MAX_NODES == 0xFFFFFFC0
    t = torch.zeros((4, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match="max_nodes"):
        V.shamap_nodes_device(t)
    with pytest.raises(ValueError, match="uint8"):
        V.shamap_nodes_device(t.to(torch.int32), max_nodes=4)
    with pytest.raises(ValueError, match="DeviceNodes"):
        V.shamap_nodes_device(t, nodes=object())
    with pytest.raises(ValueError, match="max_nodes"):
        V.HostNodes(-1)
    with pytest.raises(ValueError, match="max_nodes"):
        V.HostNodes(0xFFFFFFC1)
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        V.shamap_nodes(np.zeros((4, 20), np.uint8))
    with pytest.raises(ValueError, match="bool"):
        V.shamap_nodes(np.zeros((4, 32), np.uint8), select=np.ones(4, np.uint8))
    h = V.HostNodes(3, ids=False)
    assert h.hash.shape == (3, 32) and h.body.shape == (3, 512) and h.ids is None and h.count == 0
    s = h.struct()
    assert (s.struct_size, s.max_nodes, s.id) == (48, 3, None) and s.hash == h.hash.ctypes.data
    if not torch.cuda.is_available():
        from stellard_amd import _native as N
        with pytest.raises(N.StlError) as e:
            V.shamap_nodes(np.zeros((4, 32), np.uint8), max_nodes=4)
        assert e.value.rc == N.STL_ENODEV
