"""The fetch pack between two resident SHAMaps on the host: the model of
tests/shamap_fetch_py.py against stellard_amd/csrc/stl_shamap_fetch_core.h
compiled for the host by tests/native/hostemu_shamap_fetch.cpp.

  * the model's two statements -- the set difference over the closed form and
    the reference's stack walk with a positional hasInnerNode -- agree on the
    named and on generated pairs, with have a tree, an empty tree and none;
  * the pack's leaves are the compare's A_ONLY and CHANGED rows;
  * the rules one by one;
  * the staged call, on generations of exactly their trees' sizes, equals the
    model: nodes (hash, body, ID, meta) and the eight counts; overflow and the
    optional outputs;
  * tests/golden/shamap_fetch.json pins the model;
  * the same code in a stand-alone ASan + UBSan program (never loaded into Python);
  * the two entry points' argument checks where there is no GPU, and the Python
    wrapper's checks."""
import ctypes
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import shamap_fetch_py as FP
from tests import shamap_lookup_py as LM
from tests import shamap_nodes_py as NM
from tests import shamap_py as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emu():
    return FP.load_fetch_emu()


def _haves(have):
    return (have, {}, None)


# ---- 1. the model ----
@pytest.mark.parametrize("name", FP.PAIRS)
def test_the_two_statements_agree_on_the_named_pairs(name):
    want, have = FP.pair(name)
    for hv in _haves(have):
        diff = FP.pack_by_difference(want, hv)
        walk, _ = FP.pack_by_walk(want, hv)
        assert walk == diff, name
        if not hv:
            assert diff == NM.nodes_closed(want)  # every inner node of want
    assert FP.pack_by_difference(want, want) == {}  # equal roots: the empty pack


def test_the_two_statements_agree_on_generated_pairs():
    n = 0
    for want, have in FP.generated_pairs(300, 910):
        for hv in _haves(have):
            assert FP.pack_by_walk(want, hv)[0] == FP.pack_by_difference(want, hv)
            n += 1
    assert n == 900


def test_named_pairs_say_what_they_are_for():
    want, have = FP.pair("hash_at_other_id")
    pack = FP.pack_by_difference(want, have)
    assert len(pack) == 7 == len(NM.nodes_closed(want))
    deepest = pack[max(pack)]
    assert deepest[0] in NM.hashes_of(NM.nodes_closed(have))  # a filter keyed by hash alone would drop it
    want, have = FP.pair("same_id_other_hash")
    assert len(FP.pack_by_difference(want, have)) == 64
    want, have = FP.pair("same_id_third_key")
    assert sorted(d for d, _ in FP.pack_by_difference(want, have)) == list(range(31))
    want, have = FP.pair("bucket_have_only")
    assert all(d < 4 for d, _ in FP.pack_by_difference(want, have)) and FP.pack_by_difference(want, have)
    want, have = FP.pair("one_key")
    assert list(FP.pack_by_difference(want, have)) == [(0, bytes(32))]
    want, have = FP.pair("below_depth_10")
    assert {d for d, _ in FP.pack_by_difference(want, have)} >= set(range(11))


@pytest.mark.parametrize("name", FP.PAIRS)
def test_the_leaves_are_the_compares_a_only_and_changed_rows(name):
    want, have = FP.pair(name)
    _, leaves = FP.pack_by_walk(want, have)
    rows, _ = LM.compare(want, have, 1 << 20)
    assert leaves == {k: la for k, kind, la, _ in rows if kind in (LM.A_ONLY, LM.CHANGED)}
    assert FP.pack_by_walk(want, None)[1] == want  # against none: want's export


# ---- 2. the rules ----
def test_bucket_rows(emu):
    for differs in (0, 1):
        for cw in (0, 1, 2, 3, 70000):
            assert emu.hostemu_fetch_want_rows(differs, cw) == (cw if differs and cw >= 2 else 0)
            for ch in (0, 1, 2, 9):
                assert emu.hostemu_fetch_have_rows(differs, cw, ch) == (ch if differs and cw >= 2 and ch >= 2 else 0)


def test_top_rules(emu):
    rng = np.random.default_rng(911)
    a, b = (rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(2))
    p = LM._p
    for root in (0, 1):
        for cnt in (0, 1, 2, 5):
            assert emu.hostemu_fetch_top_inner(cnt, root) == int(cnt >= 2 or (root and cnt >= 1))
            inner = cnt >= 2 or (root and cnt >= 1)
            assert emu.hostemu_fetch_top_keeps(p(a), cnt, p(a.copy()), root) == int(not inner)
            assert emu.hostemu_fetch_top_keeps(p(a), cnt, p(b), root) == 1
    for _ in range(40):
        cnt = rng.integers(0, 3, 16).astype(np.uint32) * (rng.random(16) < 0.3)
        cnt = np.ascontiguousarray(cnt, np.uint32)
        h = rng.integers(0, 256, (16, 32), dtype=np.uint8)
        for root in (0, 1):
            assert emu.hostemu_fetch_top_value_agrees(p(cnt), p(h), root) == 1


def test_has_inner_node_rule(emu):
    """Over a hashed scratch: every node of have is held at its own ID with its own
    hash at the moment its depth has run, and not with another hash or at another ID."""
    _, have = FP.pair("cluster_bucket")
    keys, leaves = NM._sorted_arrays(have)
    l = NM._neighbours_np(keys).astype(np.int8)
    nodes = NM.nodes_closed(have)
    slot = leaves.copy()
    p = LM._p
    for d in range(63, 3, -1):
        here = {nid: v for (dd, nid), v in nodes.items() if dd == d}
        for nid, v in here.items():  # the level's launch: the slot of the node's first key
            first = next(i for i in range(len(keys)) if NM.masked(keys[i].tobytes(), d) == nid)
            slot[first] = np.frombuffer(v[0], np.uint8)
        kk, ss = np.ascontiguousarray(keys), np.ascontiguousarray(slot)
        for nid, v in here.items():
            i_d, h = np.frombuffer(nid, np.uint8).copy(), np.frombuffer(v[0], np.uint8).copy()
            assert emu.hostemu_fetch_have_holds(p(kk), p(l), p(ss), len(keys), p(i_d), d, p(h)) == 1
            other = h.copy()
            other[7] ^= 1
            assert emu.hostemu_fetch_have_holds(p(kk), p(l), p(ss), len(keys), p(i_d), d, p(other)) == 0
            away = i_d.copy()
            away[1] ^= 0x10  # another bucket: no key there
            assert emu.hostemu_fetch_have_holds(p(kk), p(l), p(ss), len(keys), p(away), d, p(h)) == 0
            assert emu.hostemu_fetch_have_holds(p(kk), p(l), p(ss), 0, p(i_d), d, p(h)) == 0


# ---- 3. the staged call against the model ----
@pytest.mark.parametrize("name", FP.PAIRS)
def test_staged_call_equals_the_model(emu, name):
    want, have = FP.pair(name)
    for hv in _haves(have):
        pack = FP.pack_by_difference(want, hv)
        out, counts = FP.emu_pack(emu, want, hv)
        assert out.guards_intact()
        assert int(out.count[0]) == len(pack)
        assert out.as_dict() == {k: v for k, v in pack.items()}
        assert counts == FP.counts(want, hv, pack), (name, hv is None)
        assert counts[4] - counts[5] == counts[0]
    out, counts = FP.emu_pack(emu, want, want)
    assert int(out.count[0]) == 0 and counts[:4] == [0, 0, 0, 0] and counts[4] == counts[5]


def test_staged_call_on_generated_pairs(emu):
    for want, have in FP.generated_pairs(60, 912):
        for hv in (have, None):
            pack = FP.pack_by_difference(want, hv)
            out, counts = FP.emu_pack(emu, want, hv)
            assert out.as_dict() == pack and counts == FP.counts(want, hv, pack)


@pytest.mark.parametrize("name", ["mixed300", "same_id_other_hash", "one_key"])
def test_overflow_and_optional_outputs(emu, name):
    want, have = FP.pair(name)
    pack = FP.pack_by_difference(want, have)
    for room in (0, len(pack) - 1):
        out, counts = FP.emu_pack(emu, want, have, max_nodes=room)
        assert out.guards_intact() and int(out.count[0]) == len(pack) == counts[0]
        got = out.as_dict()
        assert len(got) == room and all(pack[k] == v for k, v in got.items())
    out, _ = FP.emu_pack(emu, want, have, ids=False, meta=False)
    assert out.guards_intact() and int(out.count[0]) == len(pack)
    rows = int(out.count[0])
    assert sorted(h.tobytes() for h in out.hash[:rows]) == sorted(v[0] for v in pack.values())


# ---- 4. the fixture ----
def test_golden_packs(emu):
    with open(FP.GOLDEN) as f:
        doc = json.load(f)
    assert doc["packs"] == FP.golden_document()["packs"]
    assert [(p["pair"], p["against"]) for p in doc["packs"]] == [(n, a) for n in FP.GOLDEN_PAIRS
                                                                  for a in ("have", "none")]
    for p in doc["packs"]:
        want, have = FP.pair(p["pair"])
        hv = have if p["against"] == "have" else None
        out, counts = FP.emu_pack(emu, want, hv)
        got = sorted((d, nid.hex(), v[0].hex(), v[2]) for (d, nid), v in out.as_dict().items())
        assert got == [(n["depth"], n["id"], n["hash"], n["leaf_mask"]) for n in p["pack"]]
        assert counts == p["counts"]


# ---- 5. the stand-alone sanitized program ----
def test_sanitized_program(tmp_path):
    """tests/native/shamap_fetch_sanitize_main.cpp under ASan + UBSan, as a child
    process: the named pairs against the other tree and against none, with room
    for every node, for none and for one fewer."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "shamap_fetch_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("shamap_fetch_sanitize_main.cpp", "hostemu_shamap_fetch.cpp")]
    csrc = os.path.join(ROOT, "stellard_amd", "csrc")
    deps = srcs + [os.path.join(csrc, h) for h in ("stl_shamap_fetch_core.h", "stl_shamap_lookup_core.h",
                                                   "stl_shamap_tree_core.h", "stl_shamap_core.h", "stl_sha512.h",
                                                   "stl_fe25519.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0]], check=True, cwd=ROOT)
    cases = []
    for name in FP.PAIRS:
        want, have = FP.pair(name)
        for hv in (have, None):
            pack = FP.pack_by_difference(want, hv)
            for room in sorted({len(pack), 0, max(len(pack) - 1, 0)}, reverse=True):
                cases.append((want, hv, room, pack))

    def gen(items):
        ks = sorted(items)
        return struct.pack("<I", len(ks)) + b"".join(ks) + b"".join(items[k] for k in ks)

    blob = struct.pack("<I", len(cases))
    for want, hv, room, pack in cases:
        blob += gen(want) + struct.pack("<I", hv is not None) + gen(hv or {}) + struct.pack("<II", room, len(pack))
        for (d, nid), v in sorted(pack.items()):
            blob += struct.pack("<I", d) + nid + v[0]
        blob += struct.pack("<8I", *FP.counts(want, hv, pack))
    data = tmp_path / "shamap_fetch.bin"
    with open(data, "wb") as f:
        f.write(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith(f"cases {len(cases)} failed checks 0")
    assert "want 2 have 3 room 31 rc 0 nodes 31 rows 31" in r.stdout  # same_id_third_key
    assert "want 3 have none 0 room 6 rc 0 nodes 7 rows 6" in r.stdout  # hash_at_other_id, one row short


# ---- 6. the C ABI without a GPU ----
def test_argument_checks():
    """Both entry points: argument errors come before any device work, on every
    machine; a handle that is not live is STL_EINVAL with or without a device."""
    from stellard_amd import _native as N
    lib = N.load()
    buf = np.zeros(4096, np.uint8)
    base = (buf.ctypes.data + 127) & ~127
    p = lambda off=0: ctypes.c_void_p(base + off)  # noqa: E731
    fake, fake2 = ctypes.c_void_p(base + 3072), ctypes.c_void_p(base + 3200)  # never live trees

    def nodes(size=None, room=1, hash_=base, body=base + 512, ids=base + 1024, meta=base + 1536, count=base + 2048):
        return N.ShamapNodesOut(ctypes.sizeof(N.ShamapNodesOut) if size is None else size, room, hash_, body, ids,
                                meta, count)

    for device in (True, False):
        if device:
            call = lambda w, h, o, c=None: lib.stl_shamap_tree_fetch_pack_device(  # noqa: E731
                w, h, ctypes.byref(o) if o is not None else None, c, None)
        else:
            call = lambda w, h, o, c=None: lib.stl_shamap_tree_fetch_pack(  # noqa: E731
                w, h, ctypes.byref(o) if o is not None else None, c)
        assert call(None, fake2, nodes()) == N.STL_EINVAL                  # a NULL want
        assert call(None, None, nodes()) == N.STL_EINVAL
        assert call(fake, fake2, None) == N.STL_EINVAL                     # what check_nodes_out refuses
        assert call(fake, fake2, nodes(size=8)) == N.STL_EINVAL
        assert call(fake, fake2, nodes(hash_=None)) == N.STL_EINVAL
        assert call(fake, fake2, nodes(body=None)) == N.STL_EINVAL
        assert call(fake, fake2, nodes(count=None)) == N.STL_EINVAL
        assert call(fake, fake2, nodes(room=N.STL_SHAMAP_MAX_NODES + 1)) == N.STL_EINVAL
        if device:
            for off in (1, 4, 8):
                assert call(fake, fake2, nodes(hash_=base + off)) == N.STL_EINVAL
                assert call(fake, fake2, nodes(body=base + 512 + off)) == N.STL_EINVAL
                assert call(fake, fake2, nodes(ids=base + 1024 + off)) == N.STL_EINVAL
            for off in (1, 2, 3):
                assert call(fake, fake2, nodes(meta=base + 1536 + off)) == N.STL_EINVAL
                assert call(fake, fake2, nodes(count=base + 2048 + off)) == N.STL_EINVAL
                assert call(fake, fake2, nodes(), p(2560 + off)) == N.STL_EINVAL  # d_counts
        # well-formed calls on handles that are not live: against a tree, against none, against itself
        assert call(fake, fake2, nodes(), p(2560)) == N.STL_EINVAL
        assert call(fake, None, nodes(), p(2560)) == N.STL_EINVAL
        assert call(fake, fake, nodes(ids=None, meta=None)) == N.STL_EINVAL
    assert not buf.any()  # nothing was written


def test_python_wrapper_checks():
    pytest.importorskip("torch")
    from stellard_amd import verify as V

    def handle():
        t = V.ShamapTree.__new__(V.ShamapTree)  # no handle: the checks come before the library is called
        t._h = None
        return t

    want = handle()
    for fn in (want.fetch_pack_device, want.fetch_pack):
        with pytest.raises(ValueError, match="ShamapTree or None"):
            fn(object())
        with pytest.raises(ValueError, match="ShamapTree or None"):
            fn(have=5)
    with pytest.raises(ValueError, match="max_nodes"):
        want.fetch_pack_device()
    with pytest.raises(ValueError, match="max_nodes"):
        want.fetch_pack_device(handle())
    with pytest.raises(ValueError, match="DeviceNodes"):
        want.fetch_pack_device(nodes=V.HostNodes(4))
    with pytest.raises(ValueError, match="max_nodes"):
        want.fetch_pack(max_nodes=-1)
    with pytest.raises(ValueError, match="max_nodes"):
        want.fetch_pack(handle(), max_nodes=V.SHAMAP_MAX_NODES + 1)
