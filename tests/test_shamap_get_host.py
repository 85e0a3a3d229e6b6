"""A resident SHAMap's nodes by node ID and its paths by key on the host: the
model of tests/shamap_get_py.py against stellard_amd/csrc/stl_shamap_get_core.h
compiled for the host by tests/native/hostemu_shamap_get.cpp.

  * the model's two statements -- the reference's loops over the insertion tree
    and the closed form over key ranges -- agree on the named cases and on 500
    generated batches; the shapes the named cases stand for;
  * the rules one by one;
  * the staged call, on a generation of exactly its tree's size, a scratch of
    exactly the rows gathered and task arrays of exactly the tasks, equals the
    model: per request and in order; overflow and the optional outputs;
  * tests/golden/shamap_get.json pins the model;
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

from tests import shamap_get_py as GM
from tests import shamap_lookup_py as LM
from tests import shamap_nodes_py as NM
from tests import shamap_py as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emu():
    return GM.load_get_emu()


# ---- 1. the model ----
@pytest.mark.parametrize("name", GM.CASES)
def test_the_two_statements_agree_on_the_named_cases(name):
    items, requests, _ = GM.case(name)
    root = GM._tree(items)
    for nid, depth, mode in requests:
        assert GM.answer_by_walk(items, nid, depth, mode, root) == GM.answer_closed(items, nid, depth, mode)


def test_the_two_statements_agree_on_generated_batches():
    batches = seen = 0
    statuses, modes = set(), set()
    for items, requests in GM.generated_batches(510, 41):
        root, cl = GM._tree(items), GM.Closed(items)
        for nid, depth, mode in requests:
            a = cl.answer(nid, depth, mode)
            assert GM.answer_by_walk(items, nid, depth, mode, root) == a, (len(items), nid.hex(), depth, mode)
            assert len(a[1]) <= GM.MAX_ROWS
            statuses.add(a[0])
            modes.add(mode)
            seen += 1
        batches += 1
    assert batches >= 500 and seen >= 6000
    assert statuses == {GM.ABSENT, GM.INNER, GM.LEAF, GM.EMPTY_ROOT, GM.INVALID, GM.OTHER_LEAF}
    assert modes == {GM.NODE, GM.FAT, GM.PATH}


def test_what_the_named_cases_stand_for():
    def shape(name):
        items, requests, _ = GM.case(name)
        return [(st, len(rows)) for st, rows, _ in (GM.answer_closed(items, *r) for r in requests)]

    assert shape("empty") == [(GM.EMPTY_ROOT, 0), (GM.EMPTY_ROOT, 0), (GM.ABSENT, 0), (GM.ABSENT, 0), (GM.ABSENT, 0)]
    # one key: the root is one row either way, the leaf sits at depth 1, at depth 2 there is nothing;
    # the three ends of a path
    assert shape("one_key") == [(GM.INNER, 1), (GM.INNER, 1), (GM.LEAF, 0), (GM.LEAF, 0), (GM.ABSENT, 0),
                                (GM.LEAF, 1), (GM.OTHER_LEAF, 1), (GM.ABSENT, 1)]
    items, requests, _ = GM.case("one_key")
    a = GM.Answer(items, requests)
    assert bin(a.node[0][4]).count("1") == 1  # the root's leaf mask names the one leaf
    # two keys that share 63 nibbles: the chain crosses the bucket depth
    s = shape("pair63")
    assert s[0] == (GM.INNER, 64) and s[1:4] == [(GM.INNER, 1)] * 3 and s[4] == (GM.LEAF, 64) and s[5] == (GM.LEAF, 64)
    assert s[6] == (GM.INNER, 63) and s[8:10] == [(GM.INVALID, 0)] * 2 and s[10] == (GM.ABSENT, 64)
    # ... and a third key elsewhere: the root and the chain's head only; the chain and no children
    s = shape("pair63_third")
    assert s[0] == (GM.INNER, 2) and s[6] == (GM.INNER, 63)
    # 16 two-key buckets under one depth-3 prefix: the node and its 16 inner children
    assert shape("seventeen_buckets")[0] == (GM.INNER, 17)
    assert shape("seventeen_one_bucket")[1][0] == GM.INNER
    assert shape("unknown_mode") == [(GM.INVALID, 0), (GM.INVALID, 0), shape("thrice")[3], (GM.INVALID, 0)]


# ---- 2. the rules one by one ----
def test_kind_rule(emu):
    for c in range(4):
        for depth in (0, 1, 2, 5, 63):
            for parent_two in (0, 1):
                if c >= 2 or (depth == 0 and c == 1):
                    want = GM.INNER
                elif depth == 0:
                    want = GM.EMPTY_ROOT
                elif c == 1 and (depth == 1 or parent_two):
                    want = GM.LEAF
                else:
                    want = GM.ABSENT
                assert emu.hostemu_get_kind(c, depth, parent_two) == want


def test_path_rules(emu):
    assert emu.hostemu_get_path_depth(-1) == 1
    assert [emu.hostemu_get_path_depth(s) for s in (0, 1, 62, 63)] == [1, 2, 63, 64]
    for D in (1, 2, 40, 64):
        assert emu.hostemu_get_path_status(-1, D) == GM.ABSENT
        assert emu.hostemu_get_path_status(D - 1, D) == GM.ABSENT
        assert emu.hostemu_get_path_status(64, D) == GM.LEAF
        if D < 64:
            assert emu.hostemu_get_path_status(D, D) == GM.OTHER_LEAF


def test_id_masked_rule(emu):
    rng = np.random.default_rng(5)
    for _ in range(40):
        k = rng.integers(1, 256, 32, dtype=np.uint8)
        for d in (0, 1, 2, 7, 8, 9, 31, 62, 63):
            m = np.frombuffer(NM.masked(k.tobytes(), d), np.uint8).copy()
            assert emu.hostemu_get_id_masked(LM._p(m), d) == 1
            assert emu.hostemu_get_id_masked(LM._p(k), d) == 0  # every byte of k is non-zero
            m[31] |= 1
            assert emu.hostemu_get_id_masked(LM._p(m), d) == 0


def test_top_index_and_scratch_pos(emu):
    assert [emu.hostemu_get_top_index(3, t) for t in (0, 4095)] == [0, 4095]
    assert [emu.hostemu_get_top_index(2, t) for t in (0, 255)] == [4096, 4351]
    assert [emu.hostemu_get_top_index(1, t) for t in (0, 15)] == [4352, 4367]
    assert emu.hostemu_get_top_index(0, 0) == 4368
    assert emu.hostemu_get_scratch_pos(17, 12, 100) == 105


@pytest.mark.parametrize("name", ["pair63_third", "seventeen_buckets", "seventeen_one_bucket", "all_modes"])
def test_range_and_branch_end_rules(emu, name):
    items, _, _ = GM.case(name)
    g, cl = LM.EmuGen(items), GM.Closed(items)
    lo, hi = ctypes.c_uint32(), ctypes.c_uint32()
    for k in cl.keys:
        for d in (0, 1, 2, 3, 4, 5, 6, 20, 62, 63):
            nid = np.frombuffer(NM.masked(k, d), np.uint8).copy()
            emu.hostemu_get_range(LM._p(g.key), LM._p(g.bcnt), g.m, LM._p(nid), d, ctypes.byref(lo), ctypes.byref(hi))
            assert (lo.value, hi.value) == cl.range(k.hex()[:d]), (d, k.hex())
            # the end of the first key's branch of that node
            e = emu.hostemu_get_branch_end(LM._p(g.key), lo.value, hi.value, d)
            assert e == cl.range(cl.hex[lo.value][:d + 1])[1]
    # a prefix with no key
    nid = np.frombuffer(NM.masked(bytes([0xEE] * 32), 6), np.uint8).copy()
    emu.hostemu_get_range(LM._p(g.key), LM._p(g.bcnt), g.m, LM._p(nid), 6, ctypes.byref(lo), ctypes.byref(hi))
    assert lo.value == hi.value


# ---- 3. the staged call ----
@pytest.mark.parametrize("name", GM.CASES)
def test_staged_call_equals_the_model(emu, name):
    items, requests, modes = GM.case(name)
    ans = GM.Answer(items, requests)
    r = GM.emu_get(emu, items, requests, modes, total=ans.total)
    GM.check_emu(ans, r)
    # the scratch holds exactly the rows gathered, the task arrays exactly the tasks
    assert int(r.info[0]) == ans.counts[5] and int(r.info[1]) == ans.total


def test_staged_call_on_generated_batches(emu):
    for items, requests in GM.generated_batches(60, 77):
        ans = GM.Answer(items, requests)
        GM.check_emu(ans, GM.emu_get(emu, items, requests, total=ans.total))


@pytest.mark.parametrize("name", ["pair63", "seventeen_buckets", "parent_child", "all_modes"])
def test_staged_call_overflow_and_optional_outputs(emu, name):
    items, requests, modes = GM.case(name)
    nodes = NM.nodes_closed(items)
    full = GM.Answer(items, requests, nodes=nodes)
    middle = full.first[1] + max(full.rows[1] // 2, 1) if len(requests) > 1 else 1
    for room in sorted({0, full.total - 1, middle}):
        ans = GM.Answer(items, requests, max_nodes=room, nodes=nodes)
        r = GM.emu_get(emu, items, requests, modes, max_nodes=room)  # asserts that no guard is touched
        GM.check_emu(ans, r)
        assert int(r.info[1]) == min(room, full.total)
    r = GM.emu_get(emu, items, requests, modes, ids=False, meta=False, leaves=False, total=full.total)
    GM.check_emu(full, r)


# ---- 4. the fixture ----
def test_golden_answers(emu):
    with open(GM.GOLDEN) as f:
        doc = json.load(f)
    assert doc["answers"] == GM.golden_document()["answers"]
    assert [a["case"] for a in doc["answers"]] == GM.GOLDEN_CASES
    for a in doc["answers"]:
        items = {bytes.fromhex(k): bytes.fromhex(v) for k, v in a["items"]}
        requests = [(bytes.fromhex(i), d, m) for i, d, m in a["requests"]]
        assert SM.root_recursive(items)[0].hex() == a["root"]
        r = GM.emu_get(emu, items, requests, total=len(a["nodes"]))
        n = len(requests)
        assert [int(x) for x in r.status[:n]] == a["status"]
        assert [int(x) for x in r.first[:n]] == a["first"] and [int(x) for x in r.rows[:n]] == a["rows"]
        assert [bytes(k).hex() for k in r.leaf_key[:n]] == a["leaf_key"]
        assert [int(x) for x in r.counts[:8]] == a["counts"]
        got = [{"depth": int(r.out.meta[i]) & 0xFF, "id": bytes(r.out.ids[i]).hex(), "hash": bytes(r.out.hash[i]).hex(),
                "leaf_mask": int(r.out.meta[i]) >> 16} for i in range(len(a["nodes"]))]
        assert got == a["nodes"]


# ---- 5. the stand-alone sanitized program ----
def test_sanitized_program(tmp_path):
    """tests/native/shamap_get_sanitize_main.cpp under ASan + UBSan, as a child
    process: the named cases with room for every row, for none, for one fewer
    and for half of them."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "shamap_get_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("shamap_get_sanitize_main.cpp", "hostemu_shamap_get.cpp")]
    csrc = os.path.join(ROOT, "stellard_amd", "csrc")
    deps = srcs + [os.path.join(csrc, h) for h in ("stl_shamap_get_core.h", "stl_shamap_fetch_core.h",
                                                   "stl_shamap_lookup_core.h", "stl_shamap_tree_core.h",
                                                   "stl_shamap_core.h", "stl_sha512.h", "stl_fe25519.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0]], check=True, cwd=ROOT)
    cases = []
    for name in GM.CASES:
        items, requests, modes = GM.case(name)
        nodes = NM.nodes_closed(items)
        total = GM.Answer(items, requests, nodes=nodes).total
        for room in sorted({total, 0, max(total - 1, 0), total // 2}, reverse=True):
            cases.append((items, requests, modes, GM.Answer(items, requests, max_nodes=room, nodes=nodes)))
    blob = struct.pack("<I", len(cases))
    for items, requests, modes, ans in cases:
        ks = sorted(items)
        rid, rdepth, rmode = GM.request_arrays(requests)
        n = len(requests)
        blob += struct.pack("<I", len(ks)) + b"".join(ks) + b"".join(items[k] for k in ks)
        blob += struct.pack("<I", n) + rid.tobytes() + rdepth.tobytes()
        blob += struct.pack("<I", int(modes)) + rmode.tobytes()
        blob += struct.pack("<I", ans.max_nodes) + bytes(ans.status) + struct.pack(f"<{n}I", *ans.first)
        blob += struct.pack(f"<{n}I", *ans.rows) + struct.pack("<I", ans.total)
        for d, nid, h, _, _ in ans.node[:ans.max_nodes]:
            blob += struct.pack("<I", d) + nid + h
        blob += struct.pack("<8I", *ans.counts)
    data = tmp_path / "shamap_get.bin"
    with open(data, "wb") as f:
        f.write(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith(f"cases {len(cases)} failed checks 0")
    assert "items 2 requests 12 room 323 rc 0 rows 323 stored 323 scratch 2 tasks 323" in r.stdout  # pair63
    assert "items 2 requests 12 room 0 rc 0 rows 323 stored 0 scratch 0 tasks 0" in r.stdout


# ---- 6. the C ABI without a GPU ----
def test_argument_checks():
    """Both entry points: argument errors come before any device work, on every
    machine; a handle that is not live is STL_EINVAL with or without a device."""
    from stellard_amd import _native as N
    lib = N.load()
    buf = np.zeros(8192, np.uint8)
    base = (buf.ctypes.data + 127) & ~127
    p = lambda off=0: ctypes.c_void_p(base + off)  # noqa: E731
    fake = ctypes.c_void_p(base + 7168)  # never a live tree

    def nodes(size=None, room=1, hash_=base, body=base + 512, ids=base + 1024, meta=base + 1536, count=base + 2048):
        return N.ShamapNodesOut(ctypes.sizeof(N.ShamapNodesOut) if size is None else size, room, hash_, body, ids,
                                meta, count)

    good = dict(t=fake, id=p(2560), depth=p(2688), mode=p(2752), n=2, status=p(2816), first=p(2880), rows=p(2944),
                leaf_key=p(3072), leaf_hash=p(3200), out=nodes(), counts=p(3328))
    for device in (True, False):
        def call(**kw):
            a = dict(good, **kw)
            args = [a["t"], a["id"], a["depth"], a["mode"], a["n"], a["status"], a["first"], a["rows"], a["leaf_key"],
                    a["leaf_hash"], ctypes.byref(a["out"]) if a["out"] is not None else None, a["counts"]]
            if device:
                return lib.stl_shamap_tree_get_nodes_device(*args, None)
            return lib.stl_shamap_tree_get_nodes(*args)

        assert call(t=None) == N.STL_EINVAL
        for name in ("id", "depth", "status", "first", "rows"):
            assert call(**{name: None}) == N.STL_EINVAL
        assert call(n=N.STL_SHAMAP_GET_MAX_REQUESTS + 1) == N.STL_EINVAL
        assert call(out=None) == N.STL_EINVAL                              # what check_nodes_out refuses
        assert call(out=nodes(size=8)) == N.STL_EINVAL
        assert call(out=nodes(hash_=None)) == N.STL_EINVAL
        assert call(out=nodes(body=None)) == N.STL_EINVAL
        assert call(out=nodes(count=None)) == N.STL_EINVAL
        assert call(out=nodes(room=N.STL_SHAMAP_MAX_NODES + 1)) == N.STL_EINVAL
        if device:
            for off in (1, 4, 8):
                assert call(id=p(2560 + off)) == N.STL_EINVAL
                assert call(leaf_key=p(3072 + off)) == N.STL_EINVAL
                assert call(leaf_hash=p(3200 + off)) == N.STL_EINVAL
                assert call(out=nodes(hash_=base + off)) == N.STL_EINVAL
            for off in (1, 2, 3):
                assert call(first=p(2880 + off)) == N.STL_EINVAL
                assert call(rows=p(2944 + off)) == N.STL_EINVAL
                assert call(counts=p(3328 + off)) == N.STL_EINVAL
        # well-formed calls on a handle that is not live: with requests, with none, without the optional arrays
        assert call() == N.STL_EINVAL
        assert call(n=0) == N.STL_EINVAL
        assert call(mode=None, leaf_key=None, leaf_hash=None, counts=None) == N.STL_EINVAL
    assert not buf.any()  # nothing was written


def test_python_wrapper_checks():
    torch = pytest.importorskip("torch")
    from stellard_amd import verify as V

    t = V.ShamapTree.__new__(V.ShamapTree)  # no handle: the checks come before the library is called
    t._h = None
    ids = torch.zeros((3, 32), dtype=torch.uint8)
    depths = torch.zeros(3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="ids must be"):
        t.get_nodes_device(torch.zeros(3, dtype=torch.uint8), depths, max_nodes=4)
    with pytest.raises(ValueError, match="ids must be"):
        t.get_nodes_device(torch.zeros((3, 31), dtype=torch.uint8), depths, max_nodes=4)
    with pytest.raises(ValueError, match="depths must be"):
        t.get_nodes_device(ids, torch.zeros(2, dtype=torch.uint8), max_nodes=4)
    with pytest.raises(ValueError, match="modes must be"):
        t.get_nodes_device(ids, depths, torch.zeros(3, dtype=torch.int32), max_nodes=4)
    with pytest.raises(ValueError, match="max_nodes"):
        t.get_nodes_device(ids, depths)
    with pytest.raises(ValueError, match="DeviceNodes"):
        t.get_nodes_device(ids, depths, nodes=V.HostNodes(4))
    with pytest.raises(ValueError, match="ids must be"):
        t.get_nodes(np.zeros((3, 31), np.uint8), np.zeros(3, np.uint8))
    with pytest.raises(ValueError, match="depths must be"):
        t.get_nodes(np.zeros((3, 32), np.uint8), np.zeros(4, np.uint8))
    with pytest.raises(ValueError, match="modes must be"):
        t.get_nodes(np.zeros((3, 32), np.uint8), np.zeros(3, np.uint8), np.zeros(3, np.uint32))
    with pytest.raises(ValueError, match="max_nodes"):
        t.get_nodes(np.zeros((3, 32), np.uint8), np.zeros(3, np.uint8), max_nodes=-1)
    assert (V.SHAMAP_GET_NODE, V.SHAMAP_GET_FAT, V.SHAMAP_GET_PATH) == (GM.NODE, GM.FAT, GM.PATH)
    assert (V.SHAMAP_AT_ABSENT, V.SHAMAP_AT_INNER, V.SHAMAP_AT_LEAF, V.SHAMAP_AT_EMPTY_ROOT, V.SHAMAP_AT_INVALID,
            V.SHAMAP_AT_OTHER_LEAF) == (GM.ABSENT, GM.INNER, GM.LEAF, GM.EMPTY_ROOT, GM.INVALID, GM.OTHER_LEAF)
