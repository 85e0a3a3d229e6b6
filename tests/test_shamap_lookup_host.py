"""The resident SHAMap's read-only calls on the host: the model of
tests/shamap_lookup_py.py against brute force, and against
stellard_amd/csrc/stl_shamap_lookup_core.h compiled for the host by
tests/native/hostemu_shamap_lookup.cpp.

  * the model's compare equals the differences found without any bucket rule on
    small random maps (whose leaf hashes commit to their keys), and its counts
    add up; a leaf hash that does not commit to its key shows the rule's limit,
  * each rule of the core header equals the model's: the bucket's range, the
    in-bucket search, the bucket-differs rule, the two rank formulas (a
    permutation on every bucket, also with cnt_a = 0, cnt_b = 0 and all keys
    equal), the kinds, the bucket of a slot,
  * the whole staged lookup and compare equal the model,
  * tests/golden/shamap_compare.json pins the model,
  * the same code in a stand-alone ASan + UBSan program (never loaded into Python),
  * the four entry points' argument checks where there is no GPU, and the
    Python wrapper's dtype and shape checks."""
import ctypes
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import shamap_lookup_py as LM
from tests import shamap_tree_py as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emu():
    return LM.load_lookup_emu()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _arr(b):
    return np.frombuffer(b, np.uint8).copy()


def _clustered(rng, n, heads):
    """n items whose keys start with one of `heads` two-byte prefixes: few buckets, many keys each."""
    out = {}
    for k in LM._rand(rng, n):
        k = heads[int(rng.integers(0, len(heads)))] + k[2:]
        out[k] = k[::-1]
    return out


# ---- 1. the model against brute force ----
@pytest.mark.parametrize("seed", range(8))
def test_model_equals_brute_force(seed):
    rng = np.random.default_rng(200 + seed)
    heads = [bytes([3, 7]), bytes([3, 8]), bytes([0xFF, 0xFF]), bytes([0, 0])]
    base = _clustered(rng, int(rng.integers(1, 120)), heads) if seed % 2 else {k: k for k in LM._rand(rng, 60)}
    a, b = LM.derive(base, rng, int(rng.integers(0, 6)), int(rng.integers(0, 6)), int(rng.integers(0, 6)))
    for k in list(_clustered(rng, 5, heads)):
        b[k] = k
    full, c = LM.compare(a, b, 1 << 20)
    assert full == LM.brute_compare(a, b)
    assert c[0] == len(full) == c[1] + c[2] + c[3] and c[6:] == [len(a), len(b)]
    assert c[1] == len(set(a) - set(b)) and c[2] == len(set(b) - set(a))
    touched = {TM.bucket(r[0]) for r in full}
    assert c[4] == len(touched)
    assert c[5] == sum(1 for k in a if TM.bucket(k) in touched) + sum(1 for k in b if TM.bucket(k) in touched)
    for max_rows in (0, 1, len(full) - 1, len(full), len(full) + 1):
        if max_rows >= 0:
            assert LM.compare(a, b, max_rows) == (full[:max_rows], c)
    back, cb = LM.compare(b, a, 1 << 20)
    assert [r[0] for r in back] == [r[0] for r in full] and cb[:4] == [c[0], c[2], c[1], c[3]]
    assert LM.compare(a, a, 9) == ([], [0, 0, 0, 0, 0, 0, len(a), len(a)])
    # lookup
    probes = list(a)[:20] + list(b)[:20] + LM._rand(rng, 10) + [bytes(32), b"\xff" * 32]
    found, leaf, pos = LM.lookup(a, probes)
    ks = sorted(a)
    for q, f, l, p in zip(probes, found, leaf, pos):
        assert f == (q in a) and l == (a[q] if f else LM.ZERO) and (ks[p] == q if f else p == LM.NO_ROW)


def test_the_bucket_rule_is_the_references_assumption():
    """A one-key bucket's value is the key's leaf hash: the same leaf hash under
    another key of the bucket is a difference the rule cannot see (as
    SHAMap::compare cannot) -- which no SHAMap leaf kind produces."""
    rng = np.random.default_rng(210)
    k = LM._rand(rng)[0]
    other = LM._partner(k, 10, rng)
    a, b = {k: k}, {other: k}
    assert LM.compare(a, b, 4) == ([], [0, 0, 0, 0, 0, 0, 1, 1]) and len(LM.brute_compare(a, b)) == 2
    assert LM.compare(a, {other: other}, 4)[1][:6] == [2, 1, 1, 0, 1, 2]


# ---- 2. the core against the model ----
def test_range_and_in_bucket_search(emu):
    rng = np.random.default_rng(220)
    lo, hi = ctypes.c_uint32(), ctypes.c_uint32()
    for begin, cnt, m, want in ((0, 0, 0, (0, 0)), (3, 4, 10, (3, 7)), (3, 4, 5, (3, 5)), (9, 2, 5, (5, 5)),
                                (0, 0xFFFFFFFF, 7, (0, 7)), (0xFFFFFFF0, 0xFFFFFFF0, 0x1000000, (0x1000000, 0x1000000))):
        emu.hostemu_lookup_range(begin, cnt, m, ctypes.byref(lo), ctypes.byref(hi))
        assert (lo.value, hi.value) == want
    items = _clustered(rng, 300, [bytes([3, 7]), bytes([3, 8]), bytes([0x80, 0])])
    ks = sorted(items)
    sk = _arr(b"".join(ks))
    begin = {b: sum(1 for k in ks if TM.bucket(k) < b) for b in (0x0307, 0x0308, 0x8000, 0x0306, 0xFFFF)}
    count = {b: sum(1 for k in ks if TM.bucket(k) == b) for b in begin}
    probes = ks[::7] + [k[:31] + bytes([k[31] ^ 1]) for k in ks[::11]] + list(_clustered(rng, 40, [bytes([3, 7])]))
    probes += [bytes([3, 7]) + bytes(30), bytes([3, 7]) + b"\xff" * 30, LM._partner(ks[5], 63, rng)]
    found = ctypes.c_int(-1)
    for q in probes:
        b = TM.bucket(q)
        if b not in begin:
            continue
        p = emu.hostemu_lookup_lower_bound(_p(sk), begin[b], begin[b] + count[b], _p(_arr(q)), ctypes.byref(found))
        assert p == sum(1 for k in ks if k < q) and found.value == (1 if q in items else 0)
    # an empty range answers without reading a key
    assert emu.hostemu_lookup_lower_bound(None, 0, 0, _p(_arr(ks[0])), ctypes.byref(found)) == 0 and found.value == 0
    p = emu.hostemu_lookup_lower_bound(_p(sk), 300, 300, _p(_arr(ks[0])), ctypes.byref(found))
    assert p == 300 and found.value == 0


def test_bucket_differs_and_kinds(emu):
    rng = np.random.default_rng(230)
    h = rng.integers(0, 256, 32, dtype=np.uint8)
    assert emu.hostemu_bucket_differs(2, _p(h), 2, _p(h.copy())) == 0
    assert emu.hostemu_bucket_differs(2, _p(h), 3, _p(h.copy())) == 1
    assert emu.hostemu_bucket_differs(0, _p(np.zeros(32, np.uint8)), 0, _p(np.zeros(32, np.uint8))) == 0
    for byte in range(32):  # every byte of the hash counts
        g = h.copy()
        g[byte] ^= 0x10
        assert emu.hostemu_bucket_differs(5, _p(h), 5, _p(g)) == 1
    assert [emu.hostemu_diff_kind_a(f, e) for f, e in ((0, 0), (0, 1), (1, 0), (1, 1))] == \
        [LM.A_ONLY, LM.A_ONLY, LM.CHANGED, 0]
    assert [emu.hostemu_diff_kind_b(f) for f in (0, 1)] == [LM.B_ONLY, 0]
    assert emu.hostemu_diff_rank_a(5, 3) == 8 and emu.hostemu_diff_rank_b(0, 0) == 0
    assert emu.hostemu_diff_rank_b(4, 7) == 11


@pytest.mark.parametrize("na,nb,shared", [(0, 5, 0), (5, 0, 0), (1, 1, 0), (1, 1, 1), (1, 2, 1), (7, 7, 7), (40, 33, 12),
                                          (64, 65, 0), (200, 180, 150)])
def test_ranks_are_a_permutation(emu, na, nb, shared):
    """One bucket: na keys in a, nb in b, `shared` of them in both (half with
    another leaf hash).  The slots' ranks are a permutation of 0 .. na + nb - 1,
    and read in rank order the slots are the merge of the two ranges."""
    rng = np.random.default_rng(240 + na + nb)
    head = bytes([0xAB, 0xCD])
    pool = sorted(_clustered(rng, na + nb, [head]))
    rng.shuffle(pool)
    both, only_a, only_b = pool[:shared], pool[shared:na], pool[na:na + nb - shared]
    a = {k: k for k in both + only_a}
    b = {k: (k if i % 2 else k[::-1]) for i, k in enumerate(both)}
    b.update({k: k for k in only_b})
    assert (len(a), len(b)) == (na, nb)
    ka, kb = sorted(a), sorted(b)
    pad = LM._rand(rng, 3)  # rows before and after the bucket's ranges, which no slot may name
    ga = _arr(b"".join(pad[:2] + ka + pad[2:])), _arr(b"".join(pad[:2] + [a[k] for k in ka] + pad[2:]))
    gb = _arr(b"".join(pad[:1] + kb + pad[1:])), _arr(b"".join(pad[:1] + [b[k] for k in kb] + pad[1:]))
    kind, ra, rb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    slots = {}
    for q in range(na + nb):
        r = emu.hostemu_diff_slot(_p(ga[0]), _p(ga[1]), 2, 2 + na, _p(gb[0]), _p(gb[1]), 1, 1 + nb, q,
                                  ctypes.byref(kind), ctypes.byref(ra), ctypes.byref(rb))
        assert r not in slots, "two items took the same rank"
        slots[r] = (kind.value, ra.value, rb.value)
    assert sorted(slots) == list(range(na + nb))
    merged = sorted([(k, 0) for k in ka] + [(k, 1) for k in kb])  # of a key in both, a's item first
    for r, (k, side) in enumerate(merged):
        kd, xa, xb = slots[r]
        if side == 0:
            assert xa == 2 + ka.index(k)
            assert xb == (1 + kb.index(k) if k in b else LM.NO_ROW)
            assert kd == (LM.A_ONLY if k not in b else (0 if a[k] == b[k] else LM.CHANGED))
        else:
            assert xb == 1 + kb.index(k)
            assert xa == (2 + ka.index(k) if k in a else LM.NO_ROW)
            assert kd == (0 if k in a else LM.B_ONLY)


def test_all_keys_equal(emu):
    """Both ranges hold the same keys: every pair is matched, a's item first;
    equal leaf hashes report nothing, others CHANGED."""
    rng = np.random.default_rng(250)
    ks = sorted(_clustered(rng, 30, [bytes([1, 2])]))
    sk = _arr(b"".join(ks))
    la, lb = _arr(b"".join(ks)), _arr(b"".join(k if i % 3 else k[::-1] for i, k in enumerate(ks)))
    kind, ra, rb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    for q in range(60):
        r = emu.hostemu_diff_slot(_p(sk), _p(la), 0, 30, _p(sk), _p(lb), 0, 30, q, ctypes.byref(kind),
                                  ctypes.byref(ra), ctypes.byref(rb))
        i = q % 30
        assert r == 2 * i + (q >= 30) and (ra.value, rb.value) == (i, i)
        assert kind.value == (0 if q >= 30 or i % 3 else LM.CHANGED)


def test_bucket_of_a_slot(emu):
    sz = np.zeros(TM.BUCKETS, np.uint32)
    for b, n in ((0, 2), (1, 1), (700, 5), (701, 0), (0xFFFE, 3), (0xFFFF, 1)):
        sz[b] = n
    off = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint32)
    want = [b for b in range(TM.BUCKETS) for _ in range(int(sz[b]))]
    assert [emu.hostemu_diff_bucket_of(_p(off), p) for p in range(len(want))] == want


# ---- 3. the staged calls ----
@pytest.mark.parametrize("name", LM.PAIRS)
def test_the_staged_calls_equal_the_model(emu, name):
    a, b = LM.pair(name)
    ga, gb = LM.EmuGen(a), LM.EmuGen(b)
    full, c = LM.compare(a, b, 1 << 20)
    for max_rows in sorted({0, 1, max(len(full) - 1, 0), len(full), len(full) + 1}):
        assert LM.emu_compare(emu, ga, gb, max_rows) == (full[:max_rows], c)
    rows, _ = LM.emu_compare(emu, ga, gb, len(full), leaves=False)
    assert [r[:2] for r in rows] == [r[:2] for r in full]
    assert LM.emu_compare(emu, ga, ga, 3) == ([], [0, 0, 0, 0, 0, 0, len(a), len(a)])
    rng = np.random.default_rng(260)
    for n in (0, 1, 63, 64, 65, 130):
        pool = list(a) + list(b) + LM._rand(rng, 20)
        probes = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
        assert LM.emu_lookup(emu, ga, probes) == LM.lookup(a, probes)


def test_the_staged_calls_on_one_bucket_and_many(emu):
    rng = np.random.default_rng(270)
    one = _clustered(rng, 1500, [bytes([0x3C, 0x7A])])
    a, b = LM.derive(one, rng, 40, 0, 40)
    b.update(_clustered(rng, 40, [bytes([0x3C, 0x7A])]))
    full, c = LM.compare(a, b, 1 << 20)
    assert c[:6] == [120, 40, 40, 40, 1, 3000]
    assert LM.emu_compare(emu, LM.EmuGen(a), LM.EmuGen(b), 121) == (full, c)
    many = {k: k[::-1] for k in LM._rand(rng, 3000)}
    a, b = LM.derive(many, rng, 30, 30, 30)
    full, c = LM.compare(a, b, 1 << 20)
    ga, gb = LM.EmuGen(a), LM.EmuGen(b)
    assert LM.emu_compare(emu, ga, gb, 64) == (full[:64], c) and c[0] == 90 and c[5] < 400
    probes = list(a)[::3] + list(b)[::5] + LM._rand(rng, 100)
    assert LM.emu_lookup(emu, gb, probes) == LM.lookup(b, probes)


# ---- 4. the fixture ----
def test_golden_file(emu):
    from tests.golden import make_shamap_compare as MK
    with open(LM.GOLDEN) as f:
        doc = json.load(f)
    assert [p["name"] for p in doc["pairs"]] == MK.NAMES and doc["max_rows"] == MK.MAX_ROWS
    assert sum(len(p["rows"]) for p in doc["pairs"]) == 52 and any(len(p["rows"]) > MK.MAX_ROWS for p in doc["pairs"])
    for p in doc["pairs"]:
        a, b = LM.pair(p["name"])
        assert [[k.hex(), v.hex()] for k, v in sorted(a.items())] == p["a"], p["name"]
        assert [[k.hex(), v.hex()] for k, v in sorted(b.items())] == p["b"], p["name"]
        rows, counts = LM.compare(a, b, 1 << 20)
        assert [[k.hex(), kd, xa.hex(), xb.hex()] for k, kd, xa, xb in rows] == p["rows"] and counts == p["counts"]
        er, ec = LM.emu_compare(emu, LM.EmuGen(a), LM.EmuGen(b), doc["max_rows"])
        assert ec == p["counts"] and [[k.hex(), kd, xa.hex(), xb.hex()] for k, kd, xa, xb in er] == \
            p["rows"][:doc["max_rows"]]
        q = [bytes.fromhex(x[0]) for x in p["lookup"]]
        f, l, ps = LM.emu_lookup(emu, LM.EmuGen(a), q)
        assert [[q[i].hex(), f[i], l[i].hex(), ps[i]] for i in range(len(q))] == p["lookup"]
        assert (f, l, ps) == LM.lookup(a, q)


# ---- 5. the stand-alone sanitized program ----
def _gen_blob(items):
    g = LM.EmuGen(items)
    return struct.pack("<I", g.m) + g.key.tobytes() + g.leaf.tobytes() + g.bcnt.tobytes() + g.bh.tobytes()


def test_sanitized_program(tmp_path):
    """tests/native/shamap_lookup_sanitize_main.cpp under ASan + UBSan, as a
    child process: the staged lookup and compare on exactly sized heap buffers
    over the shared pairs, a one-bucket pair and every max_rows of interest."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "shamap_lookup_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("shamap_lookup_sanitize_main.cpp", "hostemu_shamap_lookup.cpp")]
    csrc = os.path.join(ROOT, "stellard_amd", "csrc")
    deps = srcs + [os.path.join(csrc, h) for h in ("stl_shamap_lookup_core.h", "stl_shamap_tree_core.h",
                                                   "stl_shamap_core.h", "stl_sha512.h", "stl_fe25519.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0]], check=True, cwd=ROOT)
    rng = np.random.default_rng(280)
    cases = []
    for name in LM.PAIRS:
        a, b = LM.pair(name)
        d = LM.compare(a, b, 1 << 20)[1][0]
        for max_rows in sorted({0, 1, max(d - 1, 0), d, d + 1}):
            cases.append((a, b, max_rows))
    one = _clustered(rng, 800, [bytes([0x3C, 0x7A])])
    a, b = LM.derive(one, rng, 25, 0, 25)
    b.update(_clustered(rng, 25, [bytes([0x3C, 0x7A])]))
    cases.append((a, b, 76))
    ends = {bytes(32): bytes(32), b"\xff" * 32: b"\xff" * 32}
    cases.append((ends, {bytes(32): b"\x01" * 32}, 2))
    blob = struct.pack("<I", len(cases))
    for a, b, max_rows in cases:
        pool = list(a) + list(b) + LM._rand(rng, 12) + [bytes(32), b"\xff" * 32]
        probes = [pool[int(i)] for i in rng.integers(0, len(pool), int(rng.choice([0, 1, 63, 64, 65, 100])))]
        found, leaf, pos = LM.lookup(a, probes)
        blob += _gen_blob(a) + _gen_blob(b) + struct.pack("<I", len(probes)) + b"".join(probes)
        blob += b"".join(struct.pack("<B", f) + l + struct.pack("<I", p) for f, l, p in zip(found, leaf, pos))
        rows, counts = LM.compare(a, b, max_rows)
        blob += struct.pack("<I8I", max_rows, *counts)
        blob += b"".join(k + struct.pack("<B", kd) + xa + xb for k, kd, xa, xb in rows)
    data = tmp_path / "shamap_lookup.bin"
    with open(data, "wb") as f:
        f.write(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith(f"cases {len(cases)} failed checks 0")
    assert "differences 75 rows 75 buckets 1 examined 1600" in r.stdout


# ---- 6. the C ABI without a GPU ----
def test_argument_checks():
    """Argument errors come before any device work, on every machine; a handle
    that is not live is STL_EINVAL whether or not there is a device."""
    from stellard_amd import _native as N
    lib = N.load()
    buf = np.zeros(2048, np.uint8)
    base = (buf.ctypes.data + 127) & ~127
    p = lambda off=0: ctypes.c_void_p(base + off)  # noqa: E731
    fake, fake2 = ctypes.c_void_p(base + 1024), ctypes.c_void_p(base + 1280)  # never live trees
    dev, host = lib.stl_shamap_tree_lookup_device, lib.stl_shamap_tree_lookup
    # NULL tree, keys, found words
    assert dev(None, p(), 1, p(64), None, None, None) == N.STL_EINVAL
    assert dev(fake, None, 1, p(64), None, None, None) == N.STL_EINVAL
    assert dev(fake, p(), 1, None, None, None, None) == N.STL_EINVAL
    assert host(None, p(), 1, p(64), None, None) == N.STL_EINVAL
    assert host(fake, None, 1, p(64), None, None) == N.STL_EINVAL
    assert host(fake, p(), 1, None, None, None) == N.STL_EINVAL
    for n in (0xFFFFFFC1, 1 << 32, (1 << 64) - 1):
        assert dev(fake, p(), n, p(64), None, None, None) == N.STL_EINVAL
        assert host(fake, p(), n, p(64), None, None) == N.STL_EINVAL
    # alignment (device form): keys and leaf hashes 16, found words 8, positions 4
    for off in (1, 4, 8):
        assert dev(fake, p(off), 1, p(64), None, None, None) == N.STL_EINVAL, off
        assert dev(fake, p(), 1, p(64), p(128 + off), None, None) == N.STL_EINVAL, off
    for off in (1, 2, 4):
        assert dev(fake, p(), 1, p(64 + off), None, None, None) == N.STL_EINVAL, off
    for off in (1, 2, 3):
        assert dev(fake, p(), 1, p(64), None, p(256 + off), None) == N.STL_EINVAL, off
    # well-formed calls on a handle that is not live -- for n == 0 as well
    assert dev(fake, p(), 2, p(64), p(128), p(256), None) == N.STL_EINVAL
    assert dev(fake, None, 0, None, None, None, None) == N.STL_EINVAL
    assert host(fake, p(1), 2, p(65), p(129), p(257)) == N.STL_EINVAL
    assert host(fake, None, 0, None, None, None) == N.STL_EINVAL
    # compare
    cdev, chost = lib.stl_shamap_tree_compare_device, lib.stl_shamap_tree_compare
    assert ctypes.sizeof(N.ShamapDiffOut) == 48

    def out(max_rows=4, key=256, kind=512, leaf_a=384, leaf_b=640, counts=768, size=None):
        q = lambda o: None if o is None else base + o  # noqa: E731
        return N.ShamapDiffOut(ctypes.sizeof(N.ShamapDiffOut) if size is None else size, max_rows, q(key), q(kind),
                               q(leaf_a), q(leaf_b), q(counts))

    for fn, extra in ((cdev, (None,)), (chost, ())):
        assert fn(None, fake, ctypes.byref(out()), *extra) == N.STL_EINVAL
        assert fn(fake, None, ctypes.byref(out()), *extra) == N.STL_EINVAL
        assert fn(fake, fake2, None, *extra) == N.STL_EINVAL
        assert fn(fake, fake2, ctypes.byref(out(counts=None)), *extra) == N.STL_EINVAL
        assert fn(fake, fake2, ctypes.byref(out(size=40)), *extra) == N.STL_EINVAL
        assert fn(fake, fake2, ctypes.byref(out(max_rows=N.STL_SHAMAP_MAX_NODES + 1)), *extra) == N.STL_EINVAL
        assert fn(fake, fake2, ctypes.byref(out(key=None)), *extra) == N.STL_EINVAL
        assert fn(fake, fake2, ctypes.byref(out(kind=None)), *extra) == N.STL_EINVAL
        # well-formed, the handles not live; a == b; no rows wanted
        assert fn(fake, fake2, ctypes.byref(out()), *extra) == N.STL_EINVAL
        assert fn(fake, fake, ctypes.byref(out(leaf_a=None, leaf_b=None)), *extra) == N.STL_EINVAL
        assert fn(fake, fake2, ctypes.byref(out(max_rows=0, key=None, kind=None)), *extra) == N.STL_EINVAL
    for off in (1, 4, 8):
        assert cdev(fake, fake2, ctypes.byref(out(key=256 + off)), None) == N.STL_EINVAL
        assert cdev(fake, fake2, ctypes.byref(out(leaf_a=384 + off)), None) == N.STL_EINVAL
        assert cdev(fake, fake2, ctypes.byref(out(leaf_b=640 + off)), None) == N.STL_EINVAL
    for off in (1, 2, 3):
        assert cdev(fake, fake2, ctypes.byref(out(counts=768 + off)), None) == N.STL_EINVAL
    # the bench's tuning key: 0 / 1, default 1
    assert lib.stl_debug_tuning(N.STL_TUNE_SHAMAP_LOOKUP_BUCKETS, -1) == 1
    assert lib.stl_debug_tuning(N.STL_TUNE_SHAMAP_LOOKUP_BUCKETS, 2) == N.STL_EINVAL
    assert lib.stl_debug_tuning(N.STL_TUNE_SHAMAP_LOOKUP_BUCKETS, 0) == 1
    assert lib.stl_debug_tuning(N.STL_TUNE_SHAMAP_LOOKUP_BUCKETS, 1) == 0
    assert not buf.any()  # nothing was written


def test_python_wrapper_refuses_wrong_dtypes_and_shapes():
    torch = pytest.importorskip("torch")
    from stellard_amd import verify as V
    tree = V.ShamapTree.__new__(V.ShamapTree)  # no handle: the checks come before the library is called
    tree._h = None
    n = 4
    t = lambda dt=torch.uint8, w=32, rows=n: torch.zeros((rows, w), dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="uint8"):
        tree.lookup_device(t(torch.int32))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        tree.lookup_device(t(w=20))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        tree.lookup_device(torch.zeros(32 * n, dtype=torch.uint8))
    with pytest.raises(ValueError, match="int64"):
        tree.lookup_device(t(), out_words=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        tree.lookup_device(t(rows=65), out_words=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="uint8"):
        tree.lookup_device(t(), leaf_hashes=t(torch.int8))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        tree.lookup_device(t(), leaf_hashes=t(rows=n + 1))
    with pytest.raises(ValueError, match=r"int32\[n\]"):
        tree.lookup_device(t(), positions=torch.zeros(n, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"int32\[n\]"):
        tree.lookup_device(t(), positions=torch.zeros(n - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="CUDA"):
        tree.lookup_device(t())  # host tensors
    k = np.zeros((n, 32), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        tree.lookup(k.astype(np.int32))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        tree.lookup(np.zeros((n, 20), np.uint8))
    # compare
    with pytest.raises(ValueError, match="ShamapTree"):
        tree.compare_device(object(), max_rows=4)
    with pytest.raises(ValueError, match="max_rows"):
        tree.compare_device(tree)
    with pytest.raises(ValueError, match="DeviceDiff"):
        tree.compare_device(tree, diff=V.HostDiff(4))
    with pytest.raises(ValueError, match="ShamapTree"):
        tree.compare(None)
    with pytest.raises(ValueError, match="max_rows"):
        V.HostDiff(-1)
    with pytest.raises(ValueError, match="max_rows"):
        V.HostDiff(V.SHAMAP_MAX_NODES + 1)
    with pytest.raises(ValueError, match="CUDA"):
        V.DeviceDiff(4, key=t(), kind=torch.zeros(n, dtype=torch.uint8), counts=torch.zeros(8, dtype=torch.int32),
                     leaf_a=False, leaf_b=False)
    d = V.HostDiff(3, leaf_b=False)
    assert d.key.shape == (3, 32) and d.kind.shape == (3,) and d.leaf_b is None and d.counts == [0] * 8
    assert d.struct().struct_size == 48 and d.struct().max_rows == 3 and d.rows() == 0
    with pytest.raises(ValueError, match="CUDA"):
        V.DeviceDiff(4, device="cpu")
