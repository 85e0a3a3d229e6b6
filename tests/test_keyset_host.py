"""Registered signer sets (stl_keyset_*, stellard_amd/csrc/stl_comb.h) on the
host: the comb tables and the doubling-free verify the gfx950 kernels run,
compiled for the host by tests/native/hostemu_keyset.cpp.

  * table rows against independent Python arithmetic,
  * every golden vector through the keyset of its 525 distinct keys,
  * the comb's point against the Straus loop's on contrived scalars,
  * a stand-alone ASan + UBSan program (never loaded into Python),
  * the C ABI's argument checks where there is no GPU.
The geometry is read from the harness, never hard-coded."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
KEYSET_SO = os.path.join(NATIVE, "libhostemu_keyset.so")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

P = 2**255 - 19
D = (-121665 * pow(121666, P - 2, P)) % P
L = 2**252 + 27742317777372353535851937790883648493
SQRTM1 = pow(2, (P - 1) // 4, P)
ORDER8 = bytes.fromhex("c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac037a")
B_ENC = bytes([0x58]) + bytes([0x66]) * 31


def load_keyset_emu():
    from stellard_amd import build
    if not os.path.exists(KEYSET_SO):
        build.build_hostemu_keyset()
    lib = ctypes.CDLL(KEYSET_SO)
    V = ctypes.c_void_p
    lib.hostemu_bound_checks.restype = ctypes.c_uint64
    lib.hostemu_bound_violations.restype = ctypes.c_uint64
    lib.hostemu_keyset_geometry.argtypes = [V]
    lib.hostemu_keyset_table.restype = ctypes.c_uint32
    lib.hostemu_keyset_table.argtypes = [V, V]
    lib.hostemu_comb_row.restype = ctypes.c_int
    lib.hostemu_comb_row.argtypes = [V, ctypes.c_uint32, ctypes.c_uint32, V]
    lib.hostemu_comb_point.restype = ctypes.c_int
    lib.hostemu_comb_point.argtypes = [V, V, V, V]
    lib.hostemu_straus_point.restype = ctypes.c_int
    lib.hostemu_straus_point.argtypes = [V, V, V, V]
    lib.hostemu_keyset_verify_batch.restype = ctypes.c_uint64
    lib.hostemu_keyset_verify_batch.argtypes = [V, ctypes.c_uint32, V, V, V, ctypes.c_size_t, V, ctypes.c_uint32]
    return lib


def geometry(lib):
    g = (ctypes.c_uint32 * 4)()
    lib.hostemu_keyset_geometry(g)
    return {"window_bits": g[0], "windows": g[1], "rows_per_window": g[2], "row_bytes": g[3]}


def keyset_of(pk):
    """(distinct keys in first-appearance order, index of each row's key)."""
    index, keys, idx = {}, [], np.zeros(pk.shape[0], np.uint32)
    for i in range(pk.shape[0]):
        b = pk[i].tobytes()
        if b not in index:
            index[b] = len(keys)
            keys.append(pk[i])
        idx[i] = index[b]
    return np.ascontiguousarray(np.stack(keys)), idx


def emu_keyset_verify(lib, keys, idx, sig, msg, policy):
    n = sig.shape[0]
    bm = np.zeros((n + 7) // 8, np.uint8)
    B = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    viol = lib.hostemu_keyset_verify_batch(B(keys), keys.shape[0], B(idx), B(sig), B(msg), n, B(bm), policy)
    return np.unpackbits(bm, bitorder="little")[:n].astype(bool), viol


# ---- independent Python arithmetic ----
def ed_add(a, b):
    x1, y1 = a
    x2, y2 = b
    t = D * x1 * x2 * y1 * y2 % P
    x3 = (x1 * y2 + x2 * y1) * pow(1 + t, P - 2, P) % P
    y3 = (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P
    return x3, y3


def ed_mul(k, a):
    r = (0, 1)
    while k:
        if k & 1:
            r = ed_add(r, a)
        a = ed_add(a, a)
        k >>= 1
    return r


def ed_decode(enc):
    """RFC 8032 decoding with y taken mod p (as ref10 does); None off the curve."""
    v = int.from_bytes(enc, "little")
    sign, y = v >> 255, (v & ((1 << 255) - 1)) % P
    u, w = (y * y - 1) % P, (D * y * y + 1) % P
    xx = u * pow(w, P - 2, P) % P
    x = pow(xx, (P + 3) // 8, P)
    if (x * x - xx) % P:
        x = x * SQRTM1 % P
    if (x * x - xx) % P:
        return None
    if (x & 1) != sign:
        x = (P - x) % P
    return x, y


def ed_encode(pt):
    x, y = pt
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def limbs_to_int(words):
    return sum(int(w) << (29 * i) for i, w in enumerate(words[:9]))


@pytest.fixture(scope="module")
def emu():
    return load_keyset_emu()


@pytest.fixture(scope="module")
def mixed_key(golden):
    """One golden class-B8 key: an honest point plus a torsion point."""
    names = [str(x) for x in golden["class_names"]]
    rows = np.nonzero(golden["cls"] == names.index("B8_mixed_order_pk"))[0]
    return golden["pk"][rows[0]].tobytes()


def _row_cases(geo):
    W, R = geo["windows"], geo["rows_per_window"]
    # the issue's rows for the 32 x 128 geometry, scaled to whatever the harness reports
    return [(0, 1), (0, R), (1, 1), (W // 2 - 1, (77 - 1) % R + 1), (W - 1, R // 4), (W - 1, R)]


def test_rows_match_python(emu, mixed_key):
    geo = geometry(emu)
    words = geo["row_bytes"] // 4
    B = ed_decode(B_ENC)
    keys = [("5B", ed_encode(ed_mul(5, B))), ("(L-1)B", ed_encode(ed_mul(L - 1, B))), ("order 8", ORDER8),
            ("mixed", mixed_key), ("base", None)]
    for name, enc in keys:
        pt = B if enc is None else ed_decode(enc)
        assert pt is not None
        if enc is not None:  # the table is built on -A
            pt = ((P - pt[0]) % P, pt[1])
        for w, j in _row_cases(geo):
            out = (ctypes.c_uint32 * words)()
            assert emu.hostemu_comb_row(enc, w, j, out) == 0
            r = list(out)
            x, y = ed_mul(j << (geo["window_bits"] * w), pt)
            assert limbs_to_int(r[0:9]) == (y + x) % P, (name, w, j)
            assert limbs_to_int(r[9:18]) == (y - x) % P, (name, w, j)
            assert limbs_to_int(r[18:27]) == 2 * D * x * y % P, (name, w, j)
            assert max(r[:27]) < 2**29 and not any(r[27:]), (name, w, j)
    assert emu.hostemu_bound_violations() == 0


def test_undecodable_key_has_no_rows(emu, golden):
    names = [str(x) for x in golden["class_names"]]
    enc = golden["pk"][np.nonzero(golden["cls"] == names.index("B10_pk_not_on_curve"))[0][0]].tobytes()
    assert ed_decode(enc) is None
    out = (ctypes.c_uint32 * (geometry(emu)["row_bytes"] // 4))()
    assert emu.hostemu_comb_row(enc, 0, 1, out) == -1


@pytest.fixture(scope="module")
def golden_keyset(golden):
    keys, idx = keyset_of(golden["pk"])
    assert keys.shape[0] == 525 and golden["pk"].shape[0] == 2163
    assert np.array_equal(keys[idx], golden["pk"])
    return keys, idx


def test_golden_policy0(emu, golden, golden_keyset):
    keys, idx = golden_keyset
    got, viol = emu_keyset_verify(emu, keys, idx, golden["sig"], golden["msg"], 0)
    exp = golden["expected_sodium_1_0_18"].astype(bool)
    assert viol == 0 and emu.hostemu_bound_checks() > 0
    assert int(exp.sum()) == 1060
    for c in range(len(golden["class_names"])):
        m = golden["cls"] == c
        assert int(got[m].sum()) == int(exp[m].sum()), str(golden["class_names"][c])
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("policy", [1, 0 | 2, 1 | 2])
def test_golden_other_policies_match_per_signature_code(emu, golden, golden_keyset, policy):
    """Policy 1 and the raw predicate (core policy bit 1) against the
    per-signature device code on the host (hostemu_verify_batch)."""
    from tests import oracle_bind
    keys, idx = golden_keyset
    got, viol = emu_keyset_verify(emu, keys, idx, golden["sig"], golden["msg"], policy)
    assert viol == 0 and emu.hostemu_bound_checks() > 0
    ref = oracle_bind.load_hostemu()
    n = golden["sig"].shape[0]
    bm = np.zeros((n + 7) // 8, np.uint8)
    B = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert ref.hostemu_verify_batch(B(golden["sig"]), B(golden["msg"]), B(golden["pk"]), n, B(bm), policy) == 0
    exp = np.unpackbits(bm, bitorder="little")[:n].astype(bool)
    assert np.array_equal(got, exp)
    if policy == 1:
        assert np.array_equal(got, golden["expected_stellard_1_0_0_unpinned"].astype(bool))


def test_bad_index_rejects_without_a_table(emu, golden, golden_keyset):
    keys, idx = golden_keyset
    rows = np.nonzero(golden["expected_sodium_1_0_18"])[0][:8]
    idx2 = idx[rows].copy()
    idx2[3] = keys.shape[0]
    idx2[5] = 0xFFFFFFFF
    got, _ = emu_keyset_verify(emu, keys, idx2, golden["sig"][rows], golden["msg"][rows], 0)
    assert got.tolist() == [True, True, True, False, True, False, True, True]


def _scalars():
    rng = np.random.default_rng(2024)
    m253 = 2**253 - 1
    vals = [0, 1, L - 1, m253, int.from_bytes(bytes([0x80]) * 32, "little") & m253,
            int.from_bytes(bytes([0x7f]) * 32, "little") & m253, (2**256 - 1) & m253]
    vals += [int.from_bytes(rng.bytes(32), "little") & m253 for _ in range(16)]
    return vals


def test_comb_point_equals_straus_point(emu, mixed_key):
    """[S]B + [k](-A) by the comb, byte for byte the Straus loop's encoding,
    for every (k, S) pair of the contrived and random scalars."""
    B = ed_decode(B_ENC)
    vals = _scalars()
    for name, enc in (("honest", ed_encode(ed_mul(0x1234567, B))), ("mixed", mixed_key), ("order 8", ORDER8)):
        A = ed_decode(enc)
        negA = ((P - A[0]) % P, A[1])
        for i, k in enumerate(vals):
            for j, S in enumerate(vals):
                a, b = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
                kb, Sb = k.to_bytes(32, "little"), S.to_bytes(32, "little")
                assert emu.hostemu_comb_point(kb, Sb, enc, a) == 0
                assert emu.hostemu_straus_point(kb, Sb, enc, b) == 0
                assert a.raw == b.raw, (name, hex(k), hex(S))
                if i == j and i < 7:  # and both are the point itself, by independent arithmetic
                    assert a.raw == ed_encode(ed_add(ed_mul(S, B), ed_mul(k, negA))), (name, hex(k), hex(S))
    assert emu.hostemu_bound_violations() == 0


def test_sanitized_program(golden, oracle, tmp_path):
    """tests/native/keyset_sanitize_main.cpp under ASan + UBSan, as a child
    process: an honest key's and an order-8 key's tables, 16 golden rows of
    those keys (valid, bit flips, S + L, small-order key), both policies."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "keyset_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("keyset_sanitize_main.cpp", "hostemu_keyset.cpp")]
    csrc = os.path.join(ROOT, "stellard_amd", "csrc")
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0], "-lpthread"], check=True, cwd=ROOT)
    # 10 rows under an honest key (a valid golden row and nine bit flips of its
    # signature or message) and 6 under the order-8 key (identity / order-8 R,
    # S = 0 and copies of the honest signature); expected bits from the oracle
    honest = golden["pk"][0].tobytes()
    assert golden["cls"][0] == 0 and golden["expected_sodium_1_0_18"][0] == 1
    sig0, msg0 = golden["sig"][0].tobytes(), golden["msg"][0].tobytes()
    rows = [(0, sig0, msg0)]
    for k in range(9):
        sg, mg = bytearray(sig0), bytearray(msg0)
        if k % 3 == 2:
            mg[(5 * k) % 32] ^= 1 << (k % 8)
        else:
            sg[(7 * k + 32 * (k % 2)) % 64] ^= 1 << (k % 8)
        rows.append((0, bytes(sg), bytes(mg)))
    ident = bytes([1]) + bytes(31)
    for R, S in ((ident, bytes(32)), (ORDER8, bytes(32)), (ident, bytes([1]) + bytes(31)), (sig0[:32], sig0[32:]),
                 (ORDER8, sig0[32:]), (sig0[:32], bytes(32))):
        rows.append((1, R + S, msg0))
    assert len(rows) == 16
    keys = [honest, ORDER8]
    sig = np.frombuffer(b"".join(r[1] for r in rows), np.uint8).reshape(-1, 64)
    msg = np.frombuffer(b"".join(r[2] for r in rows), np.uint8).reshape(-1, 32)
    pk = np.frombuffer(b"".join(keys[r[0]] for r in rows), np.uint8).reshape(-1, 32)
    e0 = oracle.verify_batch(sig, msg, pk, policy=0)
    e1 = oracle.verify_batch(sig, msg, pk, policy=1)
    assert e0[0] and e1[0] and not e0[1:10].any()
    recs = b"".join(struct.pack("<I", r[0]) + r[1] + r[2] + bytes([int(e0[i]), int(e1[i])])
                    for i, r in enumerate(rows))
    order8 = ORDER8
    path = str(tmp_path / "rows.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", 2) + honest + order8 + recs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "keys 2 rows 16 " in r.stdout and r.stdout.strip().endswith("disagreements 0")


# ---- the C ABI without a GPU ----
def test_abi_argument_checks():
    """Argument errors come before any device work, on every machine."""
    from stellard_amd import _native as N
    lib = N.load()
    pk = bytes(32)
    h = ctypes.c_void_p(0x1234)
    assert lib.stl_keyset_create(pk, 0, 0, ctypes.byref(h)) == N.STL_EINVAL and h.value is None
    h = ctypes.c_void_p(0x1234)
    assert lib.stl_keyset_create(pk, N.STL_KEYSET_MAX_KEYS + 1, 0, ctypes.byref(h)) == N.STL_EINVAL
    assert h.value is None
    assert lib.stl_keyset_create(None, 1, 0, ctypes.byref(h)) == N.STL_EINVAL
    assert lib.stl_keyset_create(pk, 1, 0, None) == N.STL_EINVAL
    assert lib.stl_keyset_create(pk, 1, 1, ctypes.byref(h)) == N.STL_EINVAL
    lib.stl_keyset_destroy(None)
    bm = ctypes.create_string_buffer(8)
    idx = np.zeros(1, np.uint32)
    ip = idx.ctypes.data_as(ctypes.c_void_p)
    assert lib.stl_keyset_verify_batch(None, ip, bytes(64), bytes(32), 1, bm, 0) == N.STL_EINVAL
    # flags: the execution flags do not apply, and 0x40 is invalid everywhere
    for flags in (0x40, N.STL_DEDUP_KEYS, N.STL_FULL_LENGTH, N.STL_ONE_LANE, N.STL_NO_AUTO_DEDUP):
        assert lib.stl_keyset_verify_batch(ctypes.c_void_p(8), ip, bytes(64), bytes(32), 1, bm, flags) == N.STL_EINVAL
        assert lib.stl_keyset_verify_batch_device(ctypes.c_void_p(8), ip, ip, ip, 1, ip, flags, None) == N.STL_EINVAL
    # a handle that is not live
    assert lib.stl_keyset_verify_batch(ctypes.c_void_p(8), ip, bytes(64), bytes(32), 1, bm, 0) == N.STL_EINVAL
    assert lib.stl_keyset_find(ctypes.c_void_p(8), pk) == -1
    assert N.STL_KEYSET_MAX_KEYS == 4096


def test_create_without_gpu_is_enodev():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu tests")
    from stellard_amd import _native as N
    lib = N.load()
    h = ctypes.c_void_p(0x1234)
    assert lib.stl_keyset_create(bytes(32), 1, 0, ctypes.byref(h)) == N.STL_ENODEV
    assert h.value is None
