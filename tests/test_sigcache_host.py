"""The verified-ID cache on the host: stellard_amd/csrc/stl_sigcache_core.h
compiled for the host by tests/native/hostemu_sigcache.cpp, against the Python
port of the hash and the model of tests/sigcache_py.py.

  * the hash against its Python port; every ID word and the seed matter,
  * insert and probe against the model over random batches at sets_log2 0, 2
    and 10, the insert guarantee checked exactly,
  * the all-zero ID never hits and is never stored,
  * a line filled with one ID's first word and zeros hits nothing,
  * the same code in a stand-alone ASan + UBSan program (never loaded into Python),
  * the entry points' argument checks where there is no GPU, and the Python
    wrapper's dtype and shape checks."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import sigcache_py as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emu():
    return SP.load_sigcache_emu()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _ids(rows):
    return np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8).reshape(-1, 32).copy()


class EmuCache:
    def __init__(self, emu, sets_log2, seed):
        self.emu, self.h = emu, emu.hostemu_sigcache_create(sets_log2, seed)
        assert self.h
        self.sets_log2 = sets_log2

    def close(self):
        self.emu.hostemu_sigcache_destroy(self.h)

    def insert(self, rows, accept=None):
        a = _ids(rows)
        f = None if accept is None else np.ascontiguousarray(accept, dtype=np.uint8)
        self.emu.hostemu_sigcache_insert(self.h, _p(a), len(rows), None if f is None else _p(f))

    def lookup(self, rows):
        a = _ids(rows)
        hit = np.full(len(rows), 0x5A, np.uint8)
        self.emu.hostemu_sigcache_lookup(self.h, _p(a), len(rows), _p(hit))
        assert set(np.unique(hit)) <= {0, 1}
        return hit.astype(bool)

    def lines(self):
        n = 32 << self.sets_log2
        return np.ctypeslib.as_array(ctypes.cast(self.emu.hostemu_sigcache_lines(self.h),
                                                 ctypes.POINTER(ctypes.c_uint32)), (n,))


# ---- 1. the hash ----
def test_hash_equals_the_python_port(emu):
    rng = np.random.default_rng(1)
    ids = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    ids[0], ids[1] = 0, 0xFF
    for seed in (0, 1, 0xD1B54A32D192ED03):
        for row in ids:
            h = emu.hostemu_sigcache_hash(_p(row), seed)
            assert h == SP.sigcache_hash(row.tobytes(), seed)
            for k in (0, 2, 10, 16, 24):
                assert emu.hostemu_sigcache_set(h, k) == SP.set_of(row.tobytes(), seed, k) < (1 << k)
            assert emu.hostemu_sigcache_first_way(h) == SP.first_way(row.tobytes(), seed) < SP.WAYS
    # every word and the seed matter, to the set index and to the whole hash
    base = SP.sigcache_hash(bytes(32), 7)
    seen = {base}
    for w in range(8):
        h = SP.sigcache_hash(bytes(4 * w) + b"\1" + bytes(31 - 4 * w), 7)
        assert h not in seen and (h >> 32) & 0xFFFFFF != (base >> 32) & 0xFFFFFF
        seen.add(h)
    assert SP.sigcache_hash(bytes(32), 7 + (1 << 63)) != base
    assert SP.sigcache_hash(bytes(32), 8) != base
    # the sets spread: 4,096 random IDs over 1,024 sets leave no set with more than 16
    assert SP.max_set_load([r.tobytes() for r in rng.integers(0, 256, (4096, 32), dtype=np.uint8)], 5, 10) <= 16
    for k in (0, 1, 10, 24):
        assert emu.hostemu_sigcache_bytes(k) == SP.LINE_BYTES << k
    assert emu.hostemu_sigcache_create(25, 1) is None


def test_the_predicate_of_a_call():
    """A cache serves the calls whose flags give its predicate: the policy bit
    and the raw-predicate bit, nothing else."""
    from stellard_amd import _native as N
    emu = SP.load_sigcache_emu()
    assert SP.PREDICATE_MASK == N.STL_POLICY_MASK | N.STL_DEBUG_RAW_PREDICATE
    execution = N.STL_FULL_LENGTH | N.STL_DEDUP_KEYS | N.STL_NO_AUTO_DEDUP | N.STL_ONE_LANE | N.STL_REQUIRE_S_LT_L
    for pred in (0, N.STL_POLICY_STELLARD_1_0_0, N.STL_DEBUG_RAW_PREDICATE,
                 N.STL_POLICY_STELLARD_1_0_0 | N.STL_DEBUG_RAW_PREDICATE):
        assert emu.hostemu_sigcache_predicate(pred) == pred
        assert emu.hostemu_sigcache_predicate(pred | execution) == pred
    assert len({emu.hostemu_sigcache_predicate(p) for p in (0, 1, 0x80000000, 0x80000001)}) == 4


# ---- 2. insert and probe against the model ----
@pytest.mark.parametrize("sets_log2", [0, 2, 10])
def test_insert_and_probe_against_the_model(emu, sets_log2):
    rng = np.random.default_rng(40 + sets_log2)
    seed = 0x5EED + sets_log2
    c, model = EmuCache(emu, sets_log2, seed), SP.Model(sets_log2, seed)
    known = []
    strangers = [rng.bytes(32) for _ in range(64)]
    # enough IDs that some sets overflow and (at 2 and 10) others do not
    rounds, most = {0: (12, 3), 2: (12, 4), 10: (40, 120)}[sets_log2]
    try:
        for r in range(rounds):
            m = int(rng.integers(1, most + 1))
            batch = [rng.bytes(32) if not known or rng.random() < 0.8 else known[int(rng.integers(len(known)))]
                     for _ in range(m)]
            accept = (rng.random(m) < 0.75).astype(np.uint8) if r % 2 else None
            c.insert(batch, accept)
            model.insert([b for i, b in enumerate(batch) if accept is None or accept[i]])
            known += batch
            hit = c.lookup(known)
            present = {known[i] for i in np.nonzero(hit)[0]}
            assert present <= model.received()  # a row held back by its accept byte is not there
            model.check(present)
            assert not c.lookup(strangers).any()
        assert model.overfull_sets()
        if sets_log2:
            assert model.guaranteed()
        if sets_log2 == 0:  # one set: exactly four IDs, the last one among them
            assert len(present) == SP.WAYS
        # after a clear nothing is present and the guarantee starts anew
        emu.hostemu_sigcache_clear(c.h)
        model.clear()
        assert not c.lookup(known).any() and not c.lines().any()
        c.insert(known[:3])
        model.insert(known[:3])
        model.check({known[i] for i in np.nonzero(c.lookup(known))[0]})
    finally:
        c.close()


def test_ways_are_taken_from_the_hashs_way(emu):
    """Four IDs of one set land in four ways, the first in its hash's way; a
    fifth overwrites its own hash's way and nothing else."""
    seed, k = 99, 2
    rng = np.random.default_rng(5)
    ids = []
    while len(ids) < 5:
        b = rng.bytes(32)
        if SP.set_of(b, seed, k) == 1:
            ids.append(b)
    c = EmuCache(emu, k, seed)
    try:
        c.insert(ids[:1])
        line = c.lines()[32:64].copy().view(np.uint8).reshape(4, 32)
        assert line[SP.first_way(ids[0], seed)].tobytes() == ids[0] and np.count_nonzero(line.any(axis=1)) == 1
        c.insert(ids[:4] + ids[:4])  # again: nothing is stored twice
        line = c.lines()[32:64].copy().view(np.uint8).reshape(4, 32)
        assert sorted(r.tobytes() for r in line) == sorted(ids[:4])
        assert not c.lines()[:32].any() and not c.lines()[64:].any()
        c.insert(ids[4:])
        after = c.lines()[32:64].copy().view(np.uint8).reshape(4, 32)
        w = SP.first_way(ids[4], seed)
        assert after[w].tobytes() == ids[4]
        assert all(after[v].tobytes() == line[v].tobytes() for v in range(4) if v != w)
        hit = c.lookup(ids)
        assert hit.sum() == 4 and hit[4]
    finally:
        c.close()


# ---- 3. / 4. the zero ID and a half-written slot ----
@pytest.mark.parametrize("sets_log2", [0, 2])
def test_zero_id_and_half_written_slot(emu, sets_log2):
    seed = 3
    c = EmuCache(emu, sets_log2, seed)
    try:
        zero = bytes(32)
        assert not c.lookup([zero])[0]  # an empty cache is all zero: the zero ID is not in it
        c.insert([zero])
        assert not c.lookup([zero])[0] and not c.lines().any()
        # first 64 bits zero: the way would look empty, so it is never stored either
        low = bytes(8) + bytes(range(1, 25))
        c.insert([low])
        assert not c.lookup([low])[0] and not c.lines().any()
        # a line filled with one ID's first word and zeros: the claim is in, the other 24 bytes are not
        rng = np.random.default_rng(9)
        x = rng.bytes(32)
        s = SP.set_of(x, seed, sets_log2)
        lines = c.lines()
        for w in range(4):
            lines[32 * s + 8 * w: 32 * s + 8 * w + 2] = np.frombuffer(x[:8], np.uint32)
        others = [rng.bytes(32) for _ in range(200)]
        assert not c.lookup([x, zero, low] + others).any()
        # ... nor any other split of the ID between written and zero words
        for cut in range(1, 8):
            lines[32 * s: 32 * s + 32] = 0
            lines[32 * s: 32 * s + cut] = np.frombuffer(x[:4 * cut], np.uint32)
            assert not c.lookup([x])[0], cut
        # a way torn between two IDs matches neither
        y = rng.bytes(32)
        lines[32 * s: 32 * s + 8] = np.frombuffer(x[:16] + y[16:], np.uint32)
        assert not c.lookup([x, y]).any()
        lines[32 * s: 32 * s + 8] = np.frombuffer(x, np.uint32)
        assert c.lookup([x])[0]
    finally:
        c.close()


# ---- 5. the stand-alone sanitized program ----
def test_sanitized_program(tmp_path):
    """tests/native/sigcache_sanitize_main.cpp under ASan + UBSan, as a child
    process: insert and lookup on exactly sized heap buffers at sets_log2 0, 2
    and 10, with the guarantee, the zero ID, a clear and a half-written slot."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "sigcache_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("sigcache_sanitize_main.cpp", "hostemu_sigcache.cpp")]
    deps = srcs + [os.path.join(ROOT, "stellard_amd", "csrc", "stl_sigcache_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0]], check=True, cwd=ROOT)
    rng = np.random.default_rng(77)
    ids = rng.integers(0, 256, (3000, 32), dtype=np.uint8)
    ids[100:110] = ids[:10]  # repeats
    seed = 0x0123456789ABCDEF
    data = tmp_path / "sigcache.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<QI", seed, ids.shape[0]) + ids.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("failed checks 0")
    assert "log2 0: sets 1 " in r.stdout and "log2 10: sets " in r.stdout and "ids 3000" in r.stdout


# ---- 6. the C ABI without a GPU ----
def test_argument_checks():
    """Argument errors come before any device work, on every machine; without
    a device every well-formed call is STL_ENODEV."""
    import torch
    from stellard_amd import _native as N
    lib = N.load()
    assert (N.STL_SIGCACHE_MAX_SETS_LOG2, N.STL_SIGCACHE_WAYS) == (SP.MAX_SETS_LOG2, SP.WAYS)
    buf = np.zeros(512, np.uint8)
    base = (buf.ctypes.data + 127) & ~127
    p = lambda off=0: ctypes.c_void_p(base + off)  # noqa: E731
    dead = ctypes.c_void_p(base + 256)  # a handle that is not live: never dereferenced
    h = ctypes.c_void_p(1)
    T, V = N.STL_BLOB_TRANSACTION, N.STL_BLOB_VALIDATION
    # create
    assert lib.stl_sigcache_create(10, T, 0, 1, None) == N.STL_EINVAL
    assert lib.stl_sigcache_create(25, T, 0, 1, ctypes.byref(h)) == N.STL_EINVAL and h.value is None
    assert lib.stl_sigcache_create(0xFFFFFFFF, T, 0, 1, ctypes.byref(h)) == N.STL_EINVAL
    assert lib.stl_sigcache_create(10, 2, 0, 1, ctypes.byref(h)) == N.STL_EINVAL
    for bad in (N.STL_FULL_LENGTH, N.STL_DEDUP_KEYS, N.STL_ONE_LANE, N.STL_NO_AUTO_DEDUP, 0x40, 0x100, 0x40000000):
        assert lib.stl_sigcache_create(10, T, bad, 1, ctypes.byref(h)) == N.STL_EINVAL, hex(bad)
    lib.stl_sigcache_destroy(None)
    lib.stl_sigcache_destroy(dead)  # ignored
    # get_info
    info = (ctypes.c_uint32 * 10)()
    info[0] = 40
    assert lib.stl_sigcache_get_info(dead, info) == N.STL_EINVAL  # not a live handle
    assert lib.stl_sigcache_get_info(dead, None) == N.STL_EINVAL
    info[0] = 36
    assert lib.stl_sigcache_get_info(dead, info) == N.STL_EINVAL  # wrong struct_size
    # NULL handle and NULL required pointers
    assert lib.stl_sigcache_clear(None, None) == N.STL_EINVAL
    assert lib.stl_sigcache_lookup_device(None, p(), 1, p(), None) == N.STL_EINVAL
    assert lib.stl_sigcache_lookup_device(dead, None, 1, p(), None) == N.STL_EINVAL
    assert lib.stl_sigcache_lookup_device(dead, p(), 1, None, None) == N.STL_EINVAL
    hits, ver = ctypes.c_size_t(7), ctypes.c_size_t(7)
    good = [dead, p(), p(), p(), 1, p(), p(), p()]
    for i in (0, 1, 2, 3, 5, 6):  # d_id (7) may be NULL
        a = list(good)
        a[i] = None
        assert lib.stl_sigcache_signed_blob_verify_batch_device(*a, 0, None, ctypes.byref(hits),
                                                                ctypes.byref(ver)) == N.STL_EINVAL, i
        assert (hits.value, ver.value) == (0, 0)
        assert lib.stl_sigcache_signed_blob_verify_batch(*a, 0, None, None) == N.STL_EINVAL, i
    # the row limit, unknown flag bits, a misaligned ID array
    too_many = 0xFFFFFFC1
    assert lib.stl_sigcache_lookup_device(dead, p(), too_many, p(), None) == N.STL_EINVAL
    big = list(good)
    big[4] = too_many
    assert lib.stl_sigcache_signed_blob_verify_batch_device(*big, 0, None, None, None) == N.STL_EINVAL
    assert lib.stl_sigcache_signed_blob_verify_batch(*big, 0, None, None) == N.STL_EINVAL
    for bad in (0x40, 0x100, 0x40000000):
        assert lib.stl_sigcache_signed_blob_verify_batch_device(*good, bad, None, None, None) == N.STL_EINVAL
        assert lib.stl_sigcache_signed_blob_verify_batch(*good, bad, None, None) == N.STL_EINVAL
    for off in (1, 4, 8):
        assert lib.stl_sigcache_lookup_device(dead, p(off), 1, p(), None) == N.STL_EINVAL, off
        a = list(good)
        a[7] = p(off)
        assert lib.stl_sigcache_signed_blob_verify_batch_device(*a, 0, None, None, None) == N.STL_EINVAL, off
    if not torch.cuda.is_available():
        assert lib.stl_sigcache_create(10, T, 0, 1, ctypes.byref(h)) == N.STL_ENODEV and h.value is None
        assert lib.stl_sigcache_create(0, V, N.STL_POLICY_STELLARD_1_0_0 | N.STL_DEBUG_RAW_PREDICATE, 0,
                                       ctypes.byref(h)) == N.STL_ENODEV
        assert lib.stl_sigcache_clear(dead, None) == N.STL_ENODEV
        assert lib.stl_sigcache_lookup_device(dead, p(), 1, p(), None) == N.STL_ENODEV
        for flags in (0, N.STL_FULL_LENGTH | N.STL_DEDUP_KEYS, N.STL_ONE_LANE | N.STL_NO_AUTO_DEDUP):
            assert lib.stl_sigcache_signed_blob_verify_batch_device(*good, flags, None, None, None) == N.STL_ENODEV
            assert lib.stl_sigcache_signed_blob_verify_batch(*good, flags, None, None) == N.STL_ENODEV
        nid = list(good)
        nid[7] = None
        assert lib.stl_sigcache_signed_blob_verify_batch_device(*nid, 0, None, None, None) == N.STL_ENODEV
    # (a predicate that is not a live cache's: test_the_predicate_of_a_call above has the rule, and
    # tests/test_gpu_sigcache.py::test_predicate_binding the refusal, where a cache can be made)


def test_python_wrapper_refuses_wrong_dtypes_and_shapes():
    torch = pytest.importorskip("torch")
    from stellard_amd import verify as V
    assert ctypes.sizeof(V.SigCacheInfo) == 40
    assert (V.SIGCACHE_MAX_SETS_LOG2, V.SIGCACHE_WAYS) == (24, 4)
    # the checks come before the handle is used: an object without one serves
    c = V.SigCache.__new__(V.SigCache)
    c._h = None
    n = 4
    ids = lambda dt=torch.uint8, w=32, rows=n: torch.zeros((rows, w), dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="uint8"):
        c.lookup_device(ids(torch.int32))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        c.lookup_device(ids(w=20))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        c.lookup_device(torch.zeros(32 * n, dtype=torch.uint8))
    with pytest.raises(ValueError, match="int64"):
        c.lookup_device(ids(), out_words=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        c.lookup_device(ids(rows=65), out_words=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="CUDA"):
        c.lookup_device(ids())  # host tensors
    blobs = torch.zeros(64, dtype=torch.uint8)
    off = torch.zeros(n, dtype=torch.int64)
    ln = torch.zeros(n, dtype=torch.int32)
    st = torch.zeros(n, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        c.signed_blob_verify_batch_device(blobs, off, ln, out_status=torch.zeros(n, dtype=torch.int32))
    with pytest.raises(ValueError, match="uint8"):
        c.signed_blob_verify_batch_device(blobs, off, ln, out_status=st, out_ids=torch.zeros((n, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        c.signed_blob_verify_batch_device(blobs, off, ln, out_status=st, out_ids=ids(w=64))
    with pytest.raises(ValueError, match="smaller"):
        c.signed_blob_verify_batch_device(blobs, off, ln, out_status=torch.zeros(n - 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="smaller"):
        c.signed_blob_verify_batch_device(blobs, off, ln, out_status=st, out_ids=ids(rows=n - 1))
    with pytest.raises(ValueError, match="int64"):
        c.signed_blob_verify_batch_device(blobs, off, ln, out_status=st, out_words=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="uint8"):
        c.signed_blob_verify_batch_device(blobs.to(torch.int32), off, ln, out_status=st)
    with pytest.raises(ValueError, match="CUDA"):
        c.signed_blob_verify_batch_device(blobs, off, ln, out_status=st)  # host tensors
