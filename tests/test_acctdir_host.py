"""The account directory on the host: stellard_amd/csrc/stl_acctdir_core.h
compiled for the host by tests/native/hostemu_acctdir.cpp (the two launches of
an upsert run one after the other), against the Python port of the hash, a
dict model and Transactor::checkSig as tests/acctdir_py.py restates it.

  * the hash against its Python port,
  * the decision function on the full cross product of its inputs,
  * insert and probe against the model over random batches, capacities 1, 5, 300,
  * 64 IDs that share one home slot, with and without a wrapped run,
  * the per-row authority function on blobs of every class of signer_cases,
  * the same code in a stand-alone ASan + UBSan program (never loaded into Python),
  * the entry points' argument checks where there is no GPU, and the Python
    wrappers' dtype and shape checks."""
import ctypes
import itertools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import acctdir_py as AP
from tests import signer_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emu():
    return AP.load_acctdir_emu()


@pytest.fixture(scope="module")
def cases():
    return SC.make_cases(20 * len(SC.CLASSES), 0xACC7)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class EmuDir:
    def __init__(self, emu, capacity, seed):
        self.emu, self.h = emu, emu.hostemu_acctdir_create(capacity, seed)

    def close(self):
        self.emu.hostemu_acctdir_destroy(self.h)

    def upsert(self, ids, flags, keys):
        a, k = AP.id_array(ids), AP.id_array(keys)
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        return self.emu.hostemu_acctdir_upsert(self.h, _p(a), _p(f), _p(k), len(ids))

    def lookup(self, ids, keys=True):
        a = AP.id_array(ids)
        f = np.full(len(ids), 0x5A, np.uint8)
        k = np.full((len(ids), 20), 0x5A, np.uint8)
        self.emu.hostemu_acctdir_lookup(self.h, _p(a), len(ids), _p(f), _p(k) if keys else None)
        return f, k

    def info(self):
        out = np.zeros(4, np.uint32)
        self.emu.hostemu_acctdir_info(self.h, _p(out))
        return dict(zip(("capacity", "records", "slots", "longest_probe"), (int(x) for x in out)))


# ---- 1. the hash ----
def test_hash_equals_the_python_port(emu):
    rng = np.random.default_rng(1)
    ids = rng.integers(0, 256, (1000, 20), dtype=np.uint8)
    ids[0], ids[1] = 0, 0xFF
    for seed in (0, 1, 0xD1B54A32D192ED03):
        for row in ids:
            assert emu.hostemu_acctdir_hash(_p(row), seed) == AP.acctdir_hash(row.tobytes(), seed)
    # every word and the seed matter
    base = AP.acctdir_hash(bytes(20), 7)
    for w in range(5):
        assert AP.acctdir_hash(bytes(4 * w) + b"\1" + bytes(19 - 4 * w), 7) != base
    assert AP.acctdir_hash(bytes(20), 7 + (1 << 63)) != base
    for cap, want in ((1, 4), (2, 8), (5, 32), (64, 256), (300, 2048), (1 << 24, 1 << 26)):
        assert emu.hostemu_acctdir_slots(cap) == want == AP.slots_for(cap)


# ---- 2. the decision function ----
def test_decision_function_cross_product(emu):
    rng = np.random.default_rng(2)
    signer, other_account, other = rng.bytes(20), rng.bytes(20), rng.bytes(20)
    seen = set()
    n = 0
    for same, presence, has_key, disabled, key_kind in itertools.product(
            (True, False), ("present", "none", "absent"), (False, True), (False, True),
            ("signer", "account", "other", "zero")):
        account = signer if same else other_account
        key = {"signer": signer, "account": account, "other": other, "zero": bytes(20)}[key_kind]
        flags = (AP.HAS_REGULAR_KEY if has_key else 0) | (AP.MASTER_DISABLED if disabled else 0)
        if presence == "absent":
            flags |= AP.ABSENT
        entry = AP.Entry(key if has_key else None, disabled) if presence == "present" else None
        want = AP.check_sig(signer, account, entry)
        # without HAS_REGULAR_KEY the key bytes passed are stale ones: they must not matter
        got = emu.hostemu_acct_authority(signer, account, presence != "none", flags, key)
        assert got == want, (same, presence, has_key, disabled, key_kind)
        seen.add(want)
        n += 1
    assert n == 96
    assert seen == {AP.AUTH_MASTER, AP.AUTH_REGULAR, AP.AUTH_MASTER_DISABLED, AP.AUTH_BAD_AUTH,
                    AP.AUTH_BAD_AUTH_MASTER, AP.AUTH_NO_ACCOUNT}
    # the master branch comes first: RegularKey == the account's own ID does not re-enable a disabled master
    assert emu.hostemu_acct_authority(signer, signer, 1, AP.HAS_REGULAR_KEY | AP.MASTER_DISABLED,
                                      signer) == AP.AUTH_MASTER_DISABLED
    # stale key bytes equal to the signer, without HAS_REGULAR_KEY
    assert emu.hostemu_acct_authority(signer, other_account, 1, 0, signer) == AP.AUTH_BAD_AUTH_MASTER
    assert emu.hostemu_acct_authority(signer, other_account, 1, AP.HAS_REGULAR_KEY, signer) == AP.AUTH_REGULAR


# ---- 3. insert and probe ----
@pytest.mark.parametrize("capacity", [1, 5, 300])
def test_insert_and_probe_against_the_model(emu, capacity):
    rng = np.random.default_rng(30 + capacity)
    d, model = EmuDir(emu, capacity, 0x5EED + capacity), AP.Model(capacity)
    known, strangers = [], [rng.bytes(20) for _ in range(40)]
    refused = 0
    try:
        assert d.info() == dict(capacity=capacity, records=0, slots=AP.slots_for(capacity), longest_probe=0)
        for _ in range(50):
            ids, flags, keys = AP.random_batch(rng, known, int(rng.integers(1, max(2, capacity // 3 + 2))))
            before = d.lookup(known + strangers)
            ok = model.upsert(ids, flags, keys)
            rc = d.upsert(ids, flags, keys)
            assert rc == (0 if ok else -12)
            if not ok:
                refused += 1
                after = d.lookup(known + strangers)
                assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
            f, k = d.lookup(known + strangers)
            wf, wk = model.lookup_arrays(known + strangers)
            assert np.array_equal(f, wf) and np.array_equal(k, wk)
            f2, _ = d.lookup(known + strangers, keys=False)
            assert np.array_equal(f2, wf)
            info = d.info()
            assert info["records"] == len(model.state) <= capacity
            assert 1 <= info["longest_probe"] <= info["records"] or info["records"] == 0
        # batches were applied and, once the directory was nearly full, refused (a batch's IDs all
        # count against the capacity, the ones already present too)
        assert 1 <= len(model.state) <= capacity and 1 <= refused < 50
    finally:
        d.close()


def test_bad_batches_are_refused(emu):
    d = EmuDir(emu, 5, 1)
    try:
        a = [bytes(20)]
        assert d.upsert(a, [0x08], a) == -22
        assert d.upsert(a, [0x80 | AP.HAS_REGULAR_KEY], a) == -22
        ids, f = AP.id_array(a), np.array([AP.HAS_REGULAR_KEY], np.uint8)
        assert emu.hostemu_acctdir_upsert(d.h, _p(ids), _p(f), None, 1) == -22  # a key is needed
        f[0] = AP.MASTER_DISABLED
        assert emu.hostemu_acctdir_upsert(d.h, _p(ids), _p(f), None, 1) == 0
        assert d.lookup(a)[0][0] == AP.MASTER_DISABLED
    finally:
        d.close()


# ---- 4. IDs that share a home slot ----
SAME_HOME_SEED = 0x0123456789ABCDEF


@pytest.fixture(scope="module")
def same_home_sets():
    """{home: 64 IDs with that home slot in a 256-slot table}: home 0, and a
    home within 10 of the table's end (the run of 64 wraps)."""
    return {home: AP.same_home_ids(64, home, 256, SAME_HOME_SEED, 40 + home) for home in (0, 250)}


@pytest.mark.parametrize("home", [0, 250])
def test_same_home_ids(emu, same_home_sets, home):
    ids = same_home_sets[home]
    assert len(set(ids)) == 64 and all(AP.acctdir_hash(i, SAME_HOME_SEED) & 255 == home for i in ids)
    rng = np.random.default_rng(home)
    keys = [rng.bytes(20) for _ in ids]
    flags = np.full(64, AP.HAS_REGULAR_KEY, np.uint8)
    strangers = [rng.bytes(20) for _ in range(64)]
    d = EmuDir(emu, 64, SAME_HOME_SEED)
    try:
        assert d.info()["slots"] == 256
        assert d.upsert(ids, flags, keys) == 0
        assert d.info()["longest_probe"] == 64 and d.info()["records"] == 64
        f, k = d.lookup(ids)
        assert np.all(f == AP.HAS_REGULAR_KEY) and np.array_equal(k, AP.id_array(keys))
        assert np.all(d.lookup(strangers)[0] == AP.NOT_FOUND)
        assert not d.lookup(strangers)[1].any()
    finally:
        d.close()


# ---- 5. the per-row authority function ----
def test_row_function_on_every_class(emu, cases):
    ids, flags, keys, want, model = AP.corpus_entries(cases, 5)
    assert set(want) == set(range(7))
    d = EmuDir(emu, len(ids), 0xABCDEF)
    try:
        assert d.upsert(ids, flags, keys) == 0
        for i, c in enumerate(cases):
            b = np.frombuffer(c.blob, np.uint8).copy()
            sg, ac = np.zeros(20, np.uint8), np.zeros(20, np.uint8)
            st = ctypes.c_uint32(99)
            auth = emu.hostemu_acctdir_authority_row(d.h, _p(b), len(c.blob), _p(sg), _p(ac), ctypes.byref(st))
            assert (st.value, sg.tobytes(), ac.tobytes()) == (c.status, c.signer, c.account), (i, c.name)
            assert auth == want[i], (i, c.name)
    finally:
        d.close()


# ---- 6. the stand-alone sanitized program ----
def test_sanitized_program(tmp_path, cases, same_home_sets):
    """tests/native/acctdir_sanitize_main.cpp under ASan + UBSan, as a child
    process: upsert and lookup on exactly sized heap buffers (capacity 1, the
    wrapped same-home run, random batches), and the row function on every
    prefix of three blobs."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "acctdir_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("acctdir_sanitize_main.cpp", "hostemu_acctdir.cpp")]
    deps = srcs + [os.path.join(ROOT, "stellard_amd", "csrc", h) for h in
                   ("stl_acctdir_core.h", "stl_hash160.h", "stl_signer_core.h", "stl_txblob.h", "stl_sha512.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0]], check=True, cwd=ROOT)
    ids, flags, keys, want, _ = AP.corpus_entries(cases, 5)
    pick = [next(i for i, c in enumerate(cases) if c.name == name)
            for name in ("master", "sendmax_invoice", "memos_paths_master")]
    data = tmp_path / "acctdir.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<QI", SAME_HOME_SEED, 64) + b"".join(same_home_sets[250]))
        f.write(struct.pack("<I", len(ids)) + b"".join(ids) + flags.tobytes() + b"".join(keys))
        f.write(struct.pack("<I", len(pick)))
        for i in pick:
            c = cases[i]
            f.write(struct.pack("<II", len(c.blob), int(want[i])) + c.signer + c.account + c.blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("failed checks 0")
    assert "same-home 64" in r.stdout and "blobs 3" in r.stdout and f"entries {len(ids)}" in r.stdout


# ---- 7. the C ABI without a GPU ----
def test_argument_checks():
    """Argument errors come before any device work, on every machine; without
    a device every well-formed call is STL_ENODEV."""
    import torch
    from stellard_amd import _native as N
    lib = N.load()
    assert (N.STL_ACCT_HAS_REGULAR_KEY, N.STL_ACCT_MASTER_DISABLED, N.STL_ACCT_ABSENT, N.STL_ACCT_NOT_FOUND) == \
        (AP.HAS_REGULAR_KEY, AP.MASTER_DISABLED, AP.ABSENT, AP.NOT_FOUND)
    assert (N.STL_AUTH_MASTER, N.STL_AUTH_REGULAR, N.STL_AUTH_MASTER_DISABLED, N.STL_AUTH_BAD_AUTH,
            N.STL_AUTH_BAD_AUTH_MASTER, N.STL_AUTH_NO_ACCOUNT, N.STL_AUTH_UNDECIDED) == tuple(range(7))
    buf = np.zeros(256, np.uint8)
    base = (buf.ctypes.data + 15) & ~15  # a 16-byte aligned address inside buf
    p = lambda off=0: ctypes.c_void_p(base + off)  # noqa: E731
    # a handle that is not live: never dereferenced (the library keeps a registry)
    dir_ = ctypes.c_void_p(base + 128)
    h = ctypes.c_void_p(1)
    # create
    assert lib.stl_acctdir_create(16, 1, None) == N.STL_EINVAL
    assert lib.stl_acctdir_create(0, 1, ctypes.byref(h)) == N.STL_EINVAL and h.value is None
    assert lib.stl_acctdir_create(N.STL_ACCTDIR_MAX_ACCOUNTS + 1, 1, ctypes.byref(h)) == N.STL_EINVAL
    lib.stl_acctdir_destroy(None)
    lib.stl_acctdir_destroy(dir_)  # ignored
    # n == 0
    assert lib.stl_acctdir_upsert(None, None, None, None, 0) == N.STL_OK
    assert lib.stl_acctdir_lookup_device(None, None, 0, None, None, None) == N.STL_OK
    assert lib.stl_acctdir_tx_blob_authority_device(None, None, None, None, 0, None, None, None, None) == N.STL_OK
    assert lib.stl_acctdir_tx_blob_authority(None, None, None, None, 0, None, None, None) == N.STL_OK
    # NULL required pointers
    good = [dir_, p(), p(), p(), 1]
    for i in (0, 1, 2):  # regular_key (3) may be NULL: the zero flags byte needs none
        a = list(good)
        a[i] = None
        assert lib.stl_acctdir_upsert(*a) == N.STL_EINVAL, i
    good = [dir_, p(), 1, p(), p()]
    for i in (0, 1, 3):  # d_regular_key (4) may be NULL
        a = list(good)
        a[i] = None
        assert lib.stl_acctdir_lookup_device(*a, None) == N.STL_EINVAL, i
    good = [dir_, p(), p(), p(), 1, p(), p(), p()]
    for i in (0, 1, 2, 3, 7):  # d_signer_id (5) and d_account (6) may be NULL
        a = list(good)
        a[i] = None
        assert lib.stl_acctdir_tx_blob_authority_device(*a, None) == N.STL_EINVAL, i
        assert lib.stl_acctdir_tx_blob_authority(*a) == N.STL_EINVAL, i
    # the row limit
    too_many = 0xFFFFFFC1
    assert lib.stl_acctdir_upsert(dir_, p(), p(), p(), too_many) == N.STL_EINVAL
    assert lib.stl_acctdir_lookup_device(dir_, p(), too_many, p(), p(), None) == N.STL_EINVAL
    assert lib.stl_acctdir_tx_blob_authority_device(dir_, p(), p(), p(), too_many, p(), p(), p(), None) == N.STL_EINVAL
    assert lib.stl_acctdir_tx_blob_authority(dir_, p(), p(), p(), too_many, p(), p(), p()) == N.STL_EINVAL
    # misaligned ID arrays are refused
    for off in (1, 2, 3):
        assert lib.stl_acctdir_lookup_device(dir_, p(off), 1, p(), p(), None) == N.STL_EINVAL, off
        assert lib.stl_acctdir_lookup_device(dir_, p(), 1, p(), p(off), None) == N.STL_EINVAL, off
        assert lib.stl_acctdir_tx_blob_authority_device(dir_, p(), p(), p(), 1, p(off), p(), p(), None) == N.STL_EINVAL
        assert lib.stl_acctdir_tx_blob_authority_device(dir_, p(), p(), p(), 1, p(), p(off), p(), None) == N.STL_EINVAL
    # unknown flag bits, and HAS_REGULAR_KEY without keys
    for bad in (0x08, 0x10, 0x80, 0xFF):
        buf[:] = 0
        buf[base - buf.ctypes.data + 64] = bad
        assert lib.stl_acctdir_upsert(dir_, p(), p(64), p(), 1) == N.STL_EINVAL, bad
    buf[:] = 0
    buf[base - buf.ctypes.data + 64] = N.STL_ACCT_HAS_REGULAR_KEY
    assert lib.stl_acctdir_upsert(dir_, p(), p(64), None, 1) == N.STL_EINVAL
    buf[:] = 0
    if not torch.cuda.is_available():
        assert lib.stl_acctdir_create(16, 1, ctypes.byref(h)) == N.STL_ENODEV and h.value is None
        assert lib.stl_acctdir_create(16, 0, ctypes.byref(h)) == N.STL_ENODEV
        assert lib.stl_acctdir_upsert(dir_, p(), p(64), p(), 1) == N.STL_ENODEV
        assert lib.stl_acctdir_upsert(dir_, p(), p(64), None, 1) == N.STL_ENODEV
        assert lib.stl_acctdir_lookup_device(dir_, p(), 1, p(), p(), None) == N.STL_ENODEV
        assert lib.stl_acctdir_lookup_device(dir_, p(), 1, p(), None, None) == N.STL_ENODEV
        assert lib.stl_acctdir_tx_blob_authority_device(dir_, p(), p(), p(), 1, p(), p(), p(), None) == N.STL_ENODEV
        assert lib.stl_acctdir_tx_blob_authority_device(dir_, p(), p(), p(), 1, None, None, p(), None) == N.STL_ENODEV
        assert lib.stl_acctdir_tx_blob_authority(dir_, p(), p(), p(), 1, p(), p(), p()) == N.STL_ENODEV
    info = (ctypes.c_uint32 * 10)()
    info[0] = 40
    assert lib.stl_acctdir_get_info(dir_, info) == N.STL_EINVAL  # not a live handle
    assert lib.stl_acctdir_get_info(dir_, None) == N.STL_EINVAL


def test_python_wrappers_refuse_wrong_dtypes_and_shapes():
    torch = pytest.importorskip("torch")
    from stellard_amd import verify as V
    assert ctypes.sizeof(V.AcctDirInfo) == 40
    assert (V.ACCT_HAS_REGULAR_KEY, V.ACCT_MASTER_DISABLED, V.ACCT_ABSENT, V.ACCT_NOT_FOUND) == (1, 2, 4, 0xFF)
    assert (V.AUTH_MASTER, V.AUTH_REGULAR, V.AUTH_MASTER_DISABLED, V.AUTH_BAD_AUTH, V.AUTH_BAD_AUTH_MASTER,
            V.AUTH_NO_ACCOUNT, V.AUTH_UNDECIDED) == tuple(range(7))
    # the checks come before the handle is used: an object without one serves
    d = V.AccountDirectory.__new__(V.AccountDirectory)
    d._h = None
    n = 4
    ids = np.zeros((n, 20), np.uint8)
    fl = np.zeros(n, np.uint8)
    with pytest.raises(ValueError, match=r"\(m, 20\) uint8"):
        d.upsert(np.zeros((n, 21), np.uint8), fl)
    with pytest.raises(ValueError, match=r"\(m, 20\) uint8"):
        d.upsert(ids.astype(np.int32), fl)
    with pytest.raises(ValueError, match=r"\(m,\) uint8"):
        d.upsert(ids, np.zeros(n + 1, np.uint8))
    with pytest.raises(ValueError, match=r"\(m,\) uint8"):
        d.upsert(ids, fl.astype(np.uint32))
    with pytest.raises(ValueError, match=r"regular_key must be \(m, 20\) uint8"):
        d.upsert(ids, fl, np.zeros((n, 32), np.uint8))
    t_ids = lambda dt=torch.uint8, w=20, rows=n: torch.zeros((rows, w), dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="uint8"):
        d.lookup_device(t_ids(torch.int32))
    with pytest.raises(ValueError, match=r"\(n, 20\)"):
        d.lookup_device(t_ids(w=32))
    with pytest.raises(ValueError, match="uint8"):
        d.lookup_device(t_ids(), out_regular_key=t_ids(torch.int64))
    with pytest.raises(ValueError, match=r"\(n, 20\)"):
        d.lookup_device(t_ids(), out_regular_key=t_ids(rows=n + 1))
    with pytest.raises(ValueError, match="uint8"):
        d.lookup_device(t_ids(), out_flags=torch.zeros(n, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\(n,\)"):
        d.lookup_device(t_ids(), out_flags=torch.zeros(n + 1, dtype=torch.uint8))
    blobs = torch.zeros(64, dtype=torch.uint8)
    off = torch.zeros(n, dtype=torch.int64)
    ln = torch.zeros(n, dtype=torch.int32)
    with pytest.raises(ValueError, match="uint8"):
        d.tx_blob_authority_device(blobs, off, ln, out_signer_id=t_ids(torch.int32))
    with pytest.raises(ValueError, match=r"\(n, 20\)"):
        d.tx_blob_authority_device(blobs, off, ln, out_signer_id=t_ids(w=32))
    with pytest.raises(ValueError, match="uint8"):
        d.tx_blob_authority_device(blobs, off, ln, out_account=t_ids(torch.int64))
    with pytest.raises(ValueError, match=r"\(n, 20\)"):
        d.tx_blob_authority_device(blobs, off, ln, out_account=t_ids(w=5))
    with pytest.raises(ValueError, match="uint8"):
        d.tx_blob_authority_device(blobs, off, ln, out_authority=torch.zeros(n, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\(n,\)"):
        d.tx_blob_authority_device(blobs, off, ln, out_authority=torch.zeros(n + 1, dtype=torch.uint8))
