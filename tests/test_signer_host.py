"""Signer authority on the host: Hash160 (stellard_amd/csrc/stl_hash160.h) and
the per-row function of tx_signer_kernel (stl_signer_core.h), compiled for the
host by tests/native/hostemu_signer.cpp, against OpenSSL's digests
(tests/golden/hash160_vectors.json) and the pure-Python restatement
(tests/hash160_py.py).

  * the Python RIPEMD-160 against the published vectors and the fixture,
  * RippleAddress_test's fourth known answer: "masterpassphrase" -> account
    ganVp9o5emfzpwrG5QVUXqMv8AgLcdvySb (RippleAddress.cpp:824,850),
  * the header's SHA-256-of-32, RIPEMD-160-of-32 and hash160_32 on every
    fixture key,
  * the per-row function on blobs of every class of tests/signer_cases.py,
  * the same code in a stand-alone ASan + UBSan program (never loaded into
    Python), on exactly sized heap copies of truncated and corrupted blobs,
  * the new entry points' argument checks where there is no GPU."""
import ctypes
import hashlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import signer_cases as SC
from tests.hash160_py import hash160, ripemd160
from tests.test_oracle_golden import b58check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emu():
    return SC.load_signer_emu()


@pytest.fixture(scope="module")
def vectors():
    return SC.load_vectors()


@pytest.fixture(scope="module")
def cases():
    return SC.make_cases(20 * len(SC.CLASSES), 0x5167)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- 1. the Python reference ----
def test_python_ripemd160_published_vectors(vectors):
    assert ripemd160(b"").hex() == "9c1185a5c5e9fc54612808977ee8f548b2258d31"
    assert ripemd160(b"abc").hex() == "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"
    msgs = {m["ascii"]: m["ripemd160"] for m in vectors["messages"]}
    assert len(msgs) == 8 and "" in msgs and "1234567890" * 8 in msgs
    for text, want in msgs.items():
        assert ripemd160(text.encode()).hex() == want, text


def test_python_hash160_reproduces_the_fixture(vectors):
    keys = [bytes.fromhex(k) for k in vectors["keys"]]
    assert len(keys) >= 800 and len(set(keys)) == len(keys) and all(len(k) == 32 for k in keys)
    assert bytes(32) in keys and b"\xff" * 32 in keys
    for k, r, h in zip(keys, vectors["ripemd160"], vectors["hash160"]):
        assert ripemd160(k).hex() == r
        assert hash160(k).hex() == h


# ---- 2. the reference's own known answer ----
def test_masterpassphrase_account(oracle, emu):
    seed = hashlib.sha512(b"masterpassphrase").digest()[:32]
    pk, _ = oracle.keypair(seed)
    assert b58check(bytes([67]) + pk) == "pGreoXKYybde1keKZwDCv8m5V1kT6JH37pgnTUVzdMkdygTixG8"
    want = bytes.fromhex("37b1b26be3c91c55d51586c3f0e5c4b03e9cea7f")
    assert hash160(pk) == want
    assert b58check(b"\x00" + want) == "ganVp9o5emfzpwrG5QVUXqMv8AgLcdvySb"
    k = np.frombuffer(pk, np.uint8).copy()
    out = np.zeros(20, np.uint8)
    emu.hostemu_hash160_32(_p(k), 1, _p(out))
    assert out.tobytes() == want


# ---- 3. host build of the header ----
def test_header_hashes_equal_the_fixture(emu, vectors):
    keys = np.frombuffer(b"".join(bytes.fromhex(k) for k in vectors["keys"]), np.uint8).reshape(-1, 32).copy()
    n = keys.shape[0]
    for i in range(n):
        d = np.zeros(32, np.uint8)
        emu.hostemu_sha256_32(_p(keys[i]), _p(d))
        assert d.tobytes() == hashlib.sha256(keys[i].tobytes()).digest(), i
        r = np.zeros(20, np.uint8)
        emu.hostemu_ripemd160_32(_p(keys[i]), _p(r))
        assert r.tobytes().hex() == vectors["ripemd160"][i], i
    out = np.zeros((n, 20), np.uint8)
    emu.hostemu_hash160_32(_p(keys), n, _p(out))
    assert [o.tobytes().hex() for o in out] == vectors["hash160"]


# ---- 4. the per-row function ----
def test_row_function_on_every_class(emu, cases):
    """The cases are of the classes they claim to be, and the per-row function
    gives what Python computes from their fields on every one."""
    by = {}
    for c in cases:
        by.setdefault(c.name, []).append(c)
    assert set(by) == set(SC.CLASSES)
    assert all(c.authority == SC.MASTER for c in by["master"] + by["memos_paths_master"])
    for name in ("random_account", "other_key", "first_byte", "last_byte"):
        assert all(c.authority == SC.NOT_MASTER and c.status == SC.TX_OK for c in by[name])
    for c in by["first_byte"]:
        assert c.account[1:] == c.signer[1:] and c.account[0] != c.signer[0]
    for c in by["last_byte"]:
        assert c.account[:19] == c.signer[:19] and c.account[19] != c.signer[19]
    for name in ("account_19", "account_21", "account_empty"):
        assert all(c.status == SC.TX_OK and c.authority == SC.UNDECIDED for c in by[name])
    assert all(c.status == SC.TX_DEFERRED for c in by["deferred"] + by["no_account"])
    assert all(c.status == SC.TX_MALFORMED for c in by["malformed"])
    # the Account payload sits at many offsets
    assert len({c.acct_off for c in cases if c.status == SC.TX_OK and c.acct_len == 20}) >= 8
    for i, c in enumerate(cases):
        st, sg, ac, auth = SC.emu_row(emu, c.blob)
        assert (st, sg, ac, auth) == (c.status, c.signer, c.account, c.authority), (i, c.name)


def test_account_position_from_the_walk(emu, cases):
    """tx_blob_parse records the top-level Account payload; absent = 0xffffffff."""
    for c in cases:
        if c.status == SC.TX_DEFERRED:
            continue
        b = np.frombuffer(c.blob, np.uint8).copy()
        pos = np.zeros(2, np.uint32)
        emu.hostemu_signer_account_pos(_p(b), len(c.blob), _p(pos))
        assert c.blob[c.acct_off - 2] == 0x81 and c.blob[c.acct_off - 1] == c.acct_len
        assert (int(pos[0]), int(pos[1])) == (c.acct_off, c.acct_len), c.name
    short = np.zeros(40, np.uint8)
    pos = np.zeros(2, np.uint32)
    emu.hostemu_signer_account_pos(_p(short), 40, _p(pos))
    assert int(pos[1]) == 0xFFFFFFFF


# ---- 5. the stand-alone sanitized program ----
def test_sanitized_program(tmp_path, cases):
    """tests/native/signer_sanitize_main.cpp under ASan + UBSan, as a child
    process: the fixture keys, and the per-row function on every prefix of
    three blobs and on those blobs with each of their first 80 bytes set to
    0xff, each in an exactly sized heap buffer."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "signer_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("signer_sanitize_main.cpp", "hostemu_signer.cpp")]
    deps = srcs + [os.path.join(ROOT, "stellard_amd", "csrc", h) for h in
                   ("stl_hash160.h", "stl_signer_core.h", "stl_txblob.h", "stl_sha512.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0]], check=True, cwd=ROOT)
    pick = [next(c for c in cases if c.name == name) for name in ("master", "sendmax_invoice", "memos_paths_master")]
    blobs = tmp_path / "blobs.bin"
    with open(blobs, "wb") as f:
        for c in pick:
            f.write(struct.pack("<II", len(c.blob), c.authority) + c.signer + c.account + c.blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "hash160_vectors.json"), str(blobs)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("failed checks 0")
    assert "keys 8" in r.stdout and "blobs 3" in r.stdout  # it did read the fixture and the blobs


# ---- 6. the C ABI without a GPU ----
def test_argument_checks():
    """Argument errors come before any device work, on every machine; without
    a device every well-formed call is STL_ENODEV."""
    import torch
    from stellard_amd import _native as N
    lib = N.load()
    assert (N.STL_ACCOUNT_ID_BYTES, N.STL_SIGNER_NOT_MASTER, N.STL_SIGNER_MASTER, N.STL_SIGNER_UNDECIDED) == (20, 0, 1, 2)
    buf = np.zeros(256, np.uint8)
    base = (buf.ctypes.data + 15) & ~15  # a 16-byte aligned address inside buf
    p = lambda off=0: ctypes.c_void_p(base + off)  # noqa: E731
    # n == 0
    assert lib.stl_account_id_batch(None, 0, None) == N.STL_OK
    assert lib.stl_account_id_batch_device(None, 0, None, None) == N.STL_OK
    assert lib.stl_tx_blob_signer_batch_device(None, None, None, 0, None, None, None, None) == N.STL_OK
    assert lib.stl_tx_blob_signer_batch(None, None, None, 0, None, None, None) == N.STL_OK
    # NULL required pointers
    assert lib.stl_account_id_batch(None, 1, p()) == N.STL_EINVAL
    assert lib.stl_account_id_batch(p(), 1, None) == N.STL_EINVAL
    assert lib.stl_account_id_batch_device(None, 1, p(), None) == N.STL_EINVAL
    assert lib.stl_account_id_batch_device(p(), 1, None, None) == N.STL_EINVAL
    good = [p(), p(), p(), 1, p(), p(), p()]
    for i in (0, 1, 2, 4, 6):  # d_account (5) may be NULL
        a = list(good)
        a[i] = None
        assert lib.stl_tx_blob_signer_batch_device(*a, None) == N.STL_EINVAL, i
        assert lib.stl_tx_blob_signer_batch(*a) == N.STL_EINVAL, i
    # the row limit
    too_many = 0xFFFFFFC1
    assert lib.stl_account_id_batch(p(), too_many, p()) == N.STL_EINVAL
    assert lib.stl_account_id_batch_device(p(), too_many, p(), None) == N.STL_EINVAL
    assert lib.stl_tx_blob_signer_batch_device(p(), p(), p(), too_many, p(), p(), p(), None) == N.STL_EINVAL
    assert lib.stl_tx_blob_signer_batch(p(), p(), p(), too_many, p(), p(), p()) == N.STL_EINVAL
    # misaligned vector accesses are refused
    for off in (1, 2, 4, 8, 12):
        assert lib.stl_account_id_batch_device(p(off), 1, p(), None) == N.STL_EINVAL, off
    for off in (1, 2, 3):
        assert lib.stl_account_id_batch_device(p(), 1, p(off), None) == N.STL_EINVAL, off
        assert lib.stl_tx_blob_signer_batch_device(p(), p(), p(), 1, p(off), p(), p(), None) == N.STL_EINVAL, off
        assert lib.stl_tx_blob_signer_batch_device(p(), p(), p(), 1, p(), p(off), p(), None) == N.STL_EINVAL, off
    if not torch.cuda.is_available():
        assert lib.stl_account_id_batch(p(), 1, p(64)) == N.STL_ENODEV
        assert lib.stl_account_id_batch_device(p(), 1, p(64), None) == N.STL_ENODEV
        assert lib.stl_tx_blob_signer_batch_device(p(), p(), p(), 1, p(), p(), p(), None) == N.STL_ENODEV
        assert lib.stl_tx_blob_signer_batch_device(p(), p(), p(), 1, p(), None, p(), None) == N.STL_ENODEV
        assert lib.stl_tx_blob_signer_batch(p(), p(), p(), 1, p(), p(), p()) == N.STL_ENODEV


def test_python_wrappers_refuse_wrong_dtypes_and_shapes():
    torch = pytest.importorskip("torch")
    from stellard_amd import verify as V
    n = 4
    pk = torch.zeros((n, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        V.account_id_batch_device(pk.to(torch.int32))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        V.account_id_batch_device(torch.zeros((n, 33), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        V.account_id_batch_device(pk, out=torch.zeros((n, 20), dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\(n, 20\)"):
        V.account_id_batch_device(pk, out=torch.zeros((n, 32), dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\(n, 20\)"):
        V.account_id_batch_device(pk, out=torch.zeros((n + 1, 20), dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        V.account_id_batch(np.zeros((n, 31), np.uint8))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        V.account_id_batch(np.zeros((n, 32), np.int32))
    blobs = torch.zeros(64, dtype=torch.uint8)
    off = torch.zeros(n, dtype=torch.int64)
    ln = torch.zeros(n, dtype=torch.int32)
    ids = lambda dt=torch.uint8, w=20: torch.zeros((n, w), dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="uint8"):
        V.tx_blob_signer_batch_device(blobs, off, ln, out_signer_id=ids(torch.int32))
    with pytest.raises(ValueError, match=r"\(n, 20\)"):
        V.tx_blob_signer_batch_device(blobs, off, ln, out_signer_id=ids(w=32))
    with pytest.raises(ValueError, match="uint8"):
        V.tx_blob_signer_batch_device(blobs, off, ln, out_account=ids(torch.int64))
    with pytest.raises(ValueError, match=r"\(n, 20\)"):
        V.tx_blob_signer_batch_device(blobs, off, ln, out_account=ids(w=5))
    with pytest.raises(ValueError, match="uint8"):
        V.tx_blob_signer_batch_device(blobs, off, ln, out_authority=torch.zeros(n, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\(n,\)"):
        V.tx_blob_signer_batch_device(blobs, off, ln, out_authority=torch.zeros(n + 1, dtype=torch.uint8))
