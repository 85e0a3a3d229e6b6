"""The resident SHAMap's fork and revert on the host: the model of
tests/shamap_fork_py.py (a fork is the tree model copied, then applied) against
stellard_amd/csrc/stl_shamap_tree_core.h compiled for the host by
tests/native/hostemu_shamap_fork.cpp.

  * the read clamp and the snapshot's row rule, on their own,
  * the whole staged fork between trees of different capacities equals the
    model: a source of capacity 8 holding 8 items into destinations of 5, 8 and
    13, a source whose stated count exceeds its capacity, the shared sequences,
  * the snapshot with 0, 1, capacity - 1 and capacity items,
  * the revert state machine against the model,
  * tests/golden/shamap_fork.json pins the model,
  * the same code in a stand-alone ASan + UBSan program (never loaded into
    Python), source larger than destination and the reverse,
  * the five entry points' argument checks where there is no GPU, and the
    Python wrapper's checks."""
import ctypes
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import shamap_fork_py as FM
from tests import shamap_py as SM
from tests import shamap_tree_py as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emu():
    return FM.load_fork_emu()


def _loaded(emu, capacity, keys, leaves=None):
    """-> (EmuTree, ModelTree) holding the keys."""
    e, m = FM.EmuTree(emu, capacity), FM.ModelTree(capacity)
    if len(keys):
        assert e.apply(keys, leaves)[0] == 0 and m.apply(keys, leaves)
    return e, m


# ---- 1. the rules ----
def test_read_clamp_and_snapshot_rows(emu):
    for stated, cap in ((0, 1), (0, 8), (7, 8), (8, 8), (9, 8), (0xFFFFFFFF, 8), (5, 0xFFFFFFFF), (1 << 24, 1 << 24)):
        assert emu.hostemu_fork_readable(stated, cap) == min(stated, cap)
        for to in (1, 5, 8, 13, 0xFFFFFFFF):
            assert emu.hostemu_fork_snapshot_rows(stated, cap, to) == min(stated, cap, to)


# ---- 2. the staged fork against the model ----
@pytest.mark.parametrize("dcap", [5, 8, 13])
def test_fork_of_a_full_source_into_other_capacities(emu, dcap):
    """Source capacity 8 with 8 items; the destination holds 5, 8 or 13."""
    k = SM.case_keys("random20", 70)
    rng = np.random.default_rng(71)
    batches = [
        (None, None, None),                                                    # the snapshot
        (k[:3].copy(), None, np.ones(3, np.uint8)),                            # 5 remain
        (k[:4].copy(), None, np.ones(4, np.uint8)),                            # 4 remain
        (np.concatenate([k[:3], k[8:10]]), None, np.array([1, 1, 1, 0, 0], np.uint8)),  # 3 out, 2 in: 7
        (k[8:13].copy(), rng.integers(0, 256, (5, 32), dtype=np.uint8), None),  # 13
        (k[2:5].copy(), k[5:8].copy(), None),                                  # replaces: 8
        (k[8:14].copy(), None, None),                                          # 14: fits none of them
    ]
    for batch in batches:
        src, sm = _loaded(emu, 8, k[:8], k[:8][:, ::-1].copy())
        dst, dm = _loaded(emu, dcap, k[14:16])
        before, held = src.content(), dst.content()
        want, root, counts = FM.fork(sm.m, *batch)
        fits = len(want.items) <= dcap
        rc, eroot, ecounts = src.fork(dst, *batch)
        assert src.content() == before == FM.content_of(sm.m)
        if batch[0] is not None and len(batch[0]) > dcap:  # an argument check: nothing has begun
            assert rc == FM.EINVAL and dst.content() == held and dst.revert() == 0
        elif fits:
            assert rc == 0
            assert (eroot, ecounts) == (root, counts)
            assert dst.content() == FM.content_of(want)
            assert dst.revert() == 0 and dst.content() == held  # what it held is what a revert brings back
        else:
            assert rc == -1 and dst.content() == held and dst.revert() == FM.EINVAL
        src.close()
        dst.close()


@pytest.mark.parametrize("stated", [9, 12, 0xFFFFFFFF])
def test_a_stated_count_past_the_source_capacity_is_clamped(emu, stated):
    """The count word says more than the source's arrays hold: its 8 rows are read, no more."""
    k = SM.case_keys("random20", 72)
    src, sm = _loaded(emu, 8, k[:8])
    for batch in ((None, None, None), (k[6:10].copy(), None, np.array([1, 0, 0, 0], np.uint8))):
        dst = FM.EmuTree(emu, 16)
        src.state_count(stated)
        want, root, counts = FM.fork(sm.m, *batch)
        assert src.fork(dst, *batch) == (0, root, counts)
        assert dst.content() == FM.content_of(want)
        dst.close()
    src.close()


@pytest.mark.parametrize("items", [0, 1, 39, 40])
def test_snapshot(emu, items):
    """Count 0, 1, capacity - 1 and capacity; into a larger, an equal and (where it fits) a smaller tree."""
    k = SM.case_keys("random40", 73)
    src, sm = _loaded(emu, 40, k[:items], k[:items][:, ::-1].copy())
    for dcap in (64, 40, max(items, 1)):
        dst, _ = _loaded(emu, dcap, k[:1])
        rc, root, counts = src.fork(dst)
        assert (rc, root, counts) == (0, sm.m.root(), [items] + [0] * 7)
        assert dst.content() == src.content() == FM.content_of(sm.m)
        dst.close()
    if items > 1:
        dst = FM.EmuTree(emu, items - 1)
        assert src.fork(dst)[0] == -1 and dst.content()[3] == 0
        dst.close()
    src.close()


@pytest.mark.parametrize("name", TM.SEQUENCES)
def test_chains_of_forks_over_the_shared_sequences(emu, name):
    """Every step of a sequence as a fork into the other of two handles of
    different capacities; the step before stays readable."""
    trees = [FM.EmuTree(emu, 1200), FM.EmuTree(emu, 1500)]
    m = TM.Model()
    for i, b in enumerate(TM.sequence(name)):
        src, dst = trees[i & 1], trees[(i & 1) ^ 1]
        was = FM.content_of(m)
        m, root, counts = FM.fork(m, *b)
        assert src.fork(dst, *b) == (0, root, counts), (name, i)
        assert dst.content() == FM.content_of(m) and src.content() == was
    for t in trees:
        t.close()


# ---- 3. the revert state machine ----
def test_revert_state_machine(emu):
    k = SM.case_keys("random40", 74)
    ones = lambda n: np.ones(n, np.uint8)  # noqa: E731

    def same(e, m):
        return e.content() == FM.content_of(m.m)

    # a fresh tree
    e, m = FM.EmuTree(emu, 16), FM.ModelTree(16)
    assert e.revert() == FM.EINVAL and not m.revert()
    # apply, revert; a second revert is refused
    assert e.apply(k[:5])[0] == 0 and m.apply(k[:5])
    assert e.revert() == 0 and m.revert() and same(e, m) and e.content()[3] == 0
    assert e.revert() == FM.EINVAL and not m.revert()
    # apply, apply, revert, revert: one step only
    assert e.apply(k[:5])[0] == 0 and m.apply(k[:5])
    assert e.apply(k[3:9], None, ones(6))[0] == 0 and m.apply(k[3:9], None, ones(6))
    assert e.revert() == 0 and m.revert() and same(e, m) and e.content()[3] == 5
    assert e.revert() == FM.EINVAL and not m.revert() and same(e, m)
    # an apply of no rows changes nothing, the revert state included
    assert e.apply(k[5:7])[0] == 0 and m.apply(k[5:7])
    assert e.apply(k[:0])[0] == 0 and m.apply(k[:0])
    assert e.revert() == 0 and m.revert() and same(e, m) and e.content()[3] == 5
    # fork-into, then revert: what the destination held comes back; the source keeps its own state
    s, sm = _loaded(emu, 12, k[20:30])
    assert s.apply(k[30:32])[0] == 0 and sm.apply(k[30:32])
    assert s.fork(e, k[:2], None, ones(2))[0] == 0 and m.fork_from(sm, k[:2], None, ones(2)) and same(e, m)
    assert e.content()[3] == 12
    assert e.revert() == 0 and m.revert() and same(e, m) and e.content()[3] == 5
    assert s.revert() == 0 and sm.revert() and same(s, sm) and s.content()[3] == 10
    # a failed apply, then revert: refused, and the content is the last good call's
    assert e.apply(k[5:8])[0] == 0 and m.apply(k[5:8])
    assert e.apply(k[8:20])[0] == -1 and not m.apply(k[8:20])
    assert e.revert() == FM.EINVAL and not m.revert() and same(e, m) and e.content()[3] == 8
    # ... until the next good call
    assert e.apply(k[8:9])[0] == 0 and m.apply(k[8:9])
    assert e.revert() == 0 and m.revert() and same(e, m)
    # a failed fork-into likewise
    assert e.apply(k[8:9])[0] == 0 and m.apply(k[8:9])
    big, bm = _loaded(emu, 40, k[:30])
    assert big.fork(e)[0] == -1 and not m.fork_from(bm)
    assert e.revert() == FM.EINVAL and not m.revert() and same(e, m)
    for t in (e, s, big):
        t.close()


# ---- 4. the fixture ----
def test_golden_cases(emu):
    with open(FM.GOLDEN) as f:
        doc = json.load(f)
    assert [c["name"] for c in doc["cases"]] == FM.CASES
    for c in doc["cases"]:
        src, batch = FM.case(c["name"])
        dst, root, counts = FM.fork(src, *batch)
        got = (len(src.items), len(batch[0]), src.root().hex(), root.hex(), counts)
        assert got == (c["source_items"], c["rows"], c["source_root"], c["fork_root"], c["counts"]), c["name"]
        assert TM.root_by_buckets(dst.items) == root
        sk, sl = src.content()
        es, _ = _loaded(emu, max(len(src.items), 1), sk, sl)
        ed = FM.EmuTree(emu, max(len(dst.items), len(batch[0]), 1))  # what the result and the call's check need
        assert es.fork(ed, *batch) == (0, root, counts), c["name"]
        assert ed.content() == FM.content_of(dst) and es.content() == FM.content_of(src)
        es.close()
        ed.close()


# ---- 5. the stand-alone sanitized program ----
def test_sanitized_program(tmp_path):
    """tests/native/shamap_fork_sanitize_main.cpp under ASan + UBSan, as a child
    process: forks, snapshots and reverts between exactly sized trees, the
    source larger than the destination and the reverse, a source whose count
    word overstates it, and refused forks."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "shamap_fork_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("shamap_fork_sanitize_main.cpp", "hostemu_shamap_fork.cpp",
                                              "hostemu_shamap_tree.cpp")]
    csrc = os.path.join(ROOT, "stellard_amd", "csrc")
    deps = srcs + [os.path.join(csrc, h) for h in ("stl_shamap_tree_core.h", "stl_shamap_core.h", "stl_sha512.h",
                                                   "stl_fe25519.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0]], check=True, cwd=ROOT)
    rng = np.random.default_rng(75)
    k = SM.case_keys("random600", 76)
    none = (np.zeros((0, 32), np.uint8), None, None)
    dels = lambda rows: (rows.copy(), None, np.ones(len(rows), np.uint8))  # noqa: E731
    # (source capacity, its items, stated count or None, destination capacity, its items, batch)
    cases = [(8, 8, None, 5, 2, dels(k[:3])), (8, 8, None, 5, 0, dels(k[:2])),     # 6 do not fit 5
             (8, 8, None, 8, 8, none), (8, 8, None, 13, 1, (k[8:13].copy(), None, None)),
             (8, 8, None, 13, 13, (k[8:14].copy(), None, None)),                     # 14 do not fit 13
             (8, 8, 12, 16, 0, none), (8, 8, 0xFFFFFFFE, 16, 3, (k[6:10].copy(), k[:4].copy(), None)),
             (600, 500, None, 300, 7, none),                                         # a snapshot refused
             (600, 500, None, 300, 7, dels(k[:200])),                                # exactly the capacity
             (600, 500, None, 299, 7, dels(k[:200])),                                # one over
             (300, 300, None, 600, 600, (k[300:].copy(), None, None)),               # the reverse, to the brim
             (300, 0, None, 600, 600, none), (1, 1, None, 1, 0, none), (1, 0, None, 1, 1, none)]
    src0, b = FM.case("one_bucket")
    cases.append((len(src0.items), src0, None, 4 * len(src0.items), 0, b))
    src0 = TM.Model()
    src0.apply(k[:400], k[:400][:, ::-1].copy())
    cases.append((512, src0, None, 450, 20, TM._mixed_batch(rng, src0.items, 257)))
    blob, refused = struct.pack("<I", len(cases)), 0
    for scap, sitems, stated, dcap, ditems, (keys, lh, ops) in cases:
        if isinstance(sitems, TM.Model):
            sm = sitems
        else:
            sm = TM.Model()
            if sitems:
                sm.apply(k[:sitems], k[:sitems][:, ::-1].copy())
        sk, sl = sm.content()
        dm = TM.Model()
        if ditems:
            dm.apply(k[:ditems])
        dk, dl = dm.content()
        want, root, counts = FM.fork(sm, keys, lh, ops)
        fits = len(want.items) <= dcap
        refused += not fits
        after = want if fits else dm
        wk, wl = after.content()
        blob += struct.pack("<III", scap, dcap, len(sm.items)) + sk.tobytes() + sl.tobytes()
        blob += struct.pack("<II", 0xFFFFFFFF if stated is None else stated, len(dm.items)) + dk.tobytes() + dl.tobytes()
        blob += struct.pack("<IBB", len(keys), lh is not None, ops is not None) + keys.tobytes()
        if lh is not None:
            blob += lh.tobytes()
        if ops is not None:
            blob += np.ascontiguousarray(ops, np.uint8).tobytes()
        blob += struct.pack("<i", 0 if fits else -1) + root + struct.pack("<8I", *counts)
        blob += struct.pack("<I", len(after.items)) + wk.tobytes() + wl.tobytes()
    data = tmp_path / "shamap_fork.bin"
    with open(data, "wb") as f:
        f.write(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith(f"cases {len(cases)} failed checks 0")
    assert refused == 4 and r.stdout.count("rc -1") == 4
    assert "source 500 of 600 into 300, n 200 rc 0 items 300" in r.stdout
    assert "source 300 of 300 into 600, n 300 rc 0 items 600" in r.stdout


# ---- 6. the C ABI without a GPU ----
def test_argument_checks():
    """The five entry points: argument errors come before any device work, on
    every machine; a handle that is not live is STL_EINVAL with or without a device."""
    from stellard_amd import _native as N
    lib = N.load()
    buf = np.zeros(2048, np.uint8)
    base = (buf.ctypes.data + 127) & ~127
    p = lambda off=0: ctypes.c_void_p(base + off)  # noqa: E731
    fake, fake2 = ctypes.c_void_p(base + 512), ctypes.c_void_p(base + 1024)  # never live trees
    nodes = N.ShamapNodesOut(ctypes.sizeof(N.ShamapNodesOut), 0, None, None, None, None, base + 1536)
    out = ctypes.byref(nodes)
    forms = [  # (entry point, device form, trailing arguments)
        (lib.stl_shamap_tree_fork_device, True, (None,)),
        (lib.stl_shamap_tree_fork, False, ()),
        (lib.stl_shamap_tree_fork_nodes_device, True, (out, None)),
        (lib.stl_shamap_tree_fork_nodes, False, (out,)),
    ]
    for fn, device, tail in forms:
        call = lambda s, d, key, leaf, op, n, root, cnt: fn(s, d, key, leaf, op, n, root, cnt, *tail)  # noqa: E731
        # NULL source, destination, root, keys; the same handle twice
        assert call(None, fake, p(), None, None, 1, p(64), None) == N.STL_EINVAL
        assert call(fake, None, p(), None, None, 1, p(64), None) == N.STL_EINVAL
        assert call(fake, fake2, p(), None, None, 1, None, None) == N.STL_EINVAL
        assert call(fake, fake2, None, None, None, 1, p(64), None) == N.STL_EINVAL
        assert call(fake, fake, p(), None, None, 1, p(64), None) == N.STL_EINVAL
        assert call(fake, fake, None, None, None, 0, p(64), None) == N.STL_EINVAL
        for n in (N.STL_SHAMAP_MAX_ITEMS + 1, 1 << 32, (1 << 64) - 1):
            assert call(fake, fake2, p(), None, None, n, p(64), None) == N.STL_EINVAL
        if device:  # alignment: keys and leaf hashes 16, root and counts 4
            for off in (1, 4, 8):
                assert call(fake, fake2, p(off), None, None, 1, p(64), None) == N.STL_EINVAL, off
                assert call(fake, fake2, p(), p(128 + off), None, 1, p(64), None) == N.STL_EINVAL, off
            for off in (1, 2, 3):
                assert call(fake, fake2, p(), None, None, 1, p(64 + off), None) == N.STL_EINVAL, off
                assert call(fake, fake2, p(), None, None, 1, p(64), p(96 + off)) == N.STL_EINVAL, off
        # well-formed calls on handles that are not live, with rows and as a snapshot
        assert call(fake, fake2, p(), p(128), p(301), 2, p(64), p(96)) == N.STL_EINVAL
        assert call(fake, fake2, None, None, None, 0, p(64), p(96)) == N.STL_EINVAL
    # the nodes forms check their struct as the apply's do
    bad = N.ShamapNodesOut(8, 0, None, None, None, None, base + 1536)
    assert lib.stl_shamap_tree_fork_nodes_device(fake, fake2, p(), None, None, 1, p(64), None, ctypes.byref(bad),
                                                 None) == N.STL_EINVAL
    assert lib.stl_shamap_tree_fork_nodes(fake, fake2, p(), None, None, 1, p(64), None, None) == N.STL_EINVAL
    assert lib.stl_shamap_tree_revert(None) == N.STL_EINVAL
    assert lib.stl_shamap_tree_revert(fake) == N.STL_EINVAL
    assert not buf.any()  # nothing was written


def test_python_wrapper_checks():
    torch = pytest.importorskip("torch")
    from stellard_amd import verify as V

    def handle():
        t = V.ShamapTree.__new__(V.ShamapTree)  # no handle: the checks come before the library is called
        t._h = None
        return t

    src, dst = handle(), handle()
    n = 4
    t = lambda dt=torch.uint8, w=32, rows=n: torch.zeros((rows, w), dtype=dt)  # noqa: E731
    for fn in (src.fork_device, src.fork_nodes_device):
        with pytest.raises(ValueError, match="ShamapTree"):
            fn(object(), t())
        with pytest.raises(ValueError, match="itself"):
            fn(src, t())
        with pytest.raises(ValueError, match="uint8"):
            fn(dst, t(torch.int32))
        with pytest.raises(ValueError, match=r"\(n, 32\)"):
            fn(dst, t(w=20))
        with pytest.raises(ValueError, match=r"\(n, 32\)"):
            fn(dst, torch.zeros(32 * n, dtype=torch.uint8))
        with pytest.raises(ValueError, match=r"\(n, 32\)"):
            fn(dst, t(), leaf_hashes=t(rows=n - 1))
        with pytest.raises(ValueError, match=r"uint8\[n\]"):
            fn(dst, t(), ops=torch.zeros(n, dtype=torch.bool))
        with pytest.raises(ValueError, match=r"\(1, 32\)"):
            fn(dst, t(), out_root=torch.zeros(32, dtype=torch.uint8))
        with pytest.raises(ValueError, match=r"int32\[8\]"):
            fn(dst, t(), counts=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="CUDA"):
        src.fork_device(dst, t())  # host tensors
    with pytest.raises(ValueError, match="max_nodes"):
        src.fork_nodes_device(dst, t())
    k = np.zeros((n, 32), np.uint8)
    for fn in (src.fork, src.fork_nodes):
        with pytest.raises(ValueError, match="ShamapTree"):
            fn(None, k)
        with pytest.raises(ValueError, match="itself"):
            fn(src, k)
        with pytest.raises(ValueError, match="uint8"):
            fn(dst, k.astype(np.int32))
        with pytest.raises(ValueError, match=r"\(n, 32\)"):
            fn(dst, np.zeros((n, 20), np.uint8))
        with pytest.raises(ValueError, match="leaf_hashes"):
            fn(dst, k, leaf_hashes=np.zeros((n - 1, 32), np.uint8))
        with pytest.raises(ValueError, match="ops"):
            fn(dst, k, ops=np.zeros(n + 1, np.uint8))
    with pytest.raises(ValueError, match="max_nodes"):
        src.fork_nodes(dst, k, max_nodes=-1)
