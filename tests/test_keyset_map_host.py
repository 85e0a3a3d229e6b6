"""The keyset's key -> index map (stellard_amd/csrc/stl_keyset_map.h) on the
host: the builder stl_keyset_create runs and the hash and probe the gfx950
lookup kernel runs, compiled for the host by tests/native/hostemu_keyset_map.cpp.

  * random sets with duplicates: every key to its first index, strangers and
    one-bit neighbours to not-found, a power-of-two slot count >= 4 * nkeys,
  * a set made to collide under seed 0: the builder moves on to a later seed
    and keeps the probe bound,
  * the same cases in a stand-alone ASan + UBSan program (never loaded into
    Python),
  * the by-key entry points' argument checks where there is no GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
MAP_SO = os.path.join(NATIVE, "libhostemu_keyset_map.so")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NKEYS = [1, 2, 3, 255, 256, 257, 4096]


def load_map_emu():
    from stellard_amd import build
    build.build_hostemu_keyset_map()
    lib = ctypes.CDLL(MAP_SO)
    V = ctypes.c_void_p
    lib.hostemu_keyset_map_bound.restype = ctypes.c_uint32
    lib.hostemu_keyset_map_empty.restype = ctypes.c_uint32
    lib.hostemu_keyset_map_hash.restype = ctypes.c_uint32
    lib.hostemu_keyset_map_hash.argtypes = [V, ctypes.c_uint64]
    lib.hostemu_keyset_map_build.restype = V
    lib.hostemu_keyset_map_build.argtypes = [V, ctypes.c_uint32]
    lib.hostemu_keyset_map_free.argtypes = [V]
    lib.hostemu_keyset_map_info.argtypes = [V, V]
    lib.hostemu_keyset_map_probe.argtypes = [V, V, ctypes.c_size_t, V]
    return lib


@pytest.fixture(scope="module")
def emu():
    return load_map_emu()


class Map:
    def __init__(self, lib, keys):
        self.lib = lib
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
        self.h = lib.hostemu_keyset_map_build(keys.ctypes.data_as(ctypes.c_void_p), keys.shape[0])
        assert self.h, "no seed served"
        info = (ctypes.c_uint32 * 4)()
        lib.hostemu_keyset_map_info(self.h, info)
        self.slots, self.longest, self.seed = info[0], info[1], info[2] | (info[3] << 32)

    def probe(self, keys):
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 32)
        out = np.zeros(keys.shape[0], np.uint32)
        self.lib.hostemu_keyset_map_probe(self.h, keys.ctypes.data_as(ctypes.c_void_p), keys.shape[0],
                                          out.ctypes.data_as(ctypes.c_void_p))
        return out

    def close(self):
        self.lib.hostemu_keyset_map_free(self.h)


def first_index(keys):
    first, out = {}, np.zeros(keys.shape[0], np.uint32)
    for i in range(keys.shape[0]):
        out[i] = first.setdefault(keys[i].tobytes(), i)
    return out, first


def check_set(emu, keys, rng):
    """Every lookup of the set's map is right; returns the map's (slots, longest, seed)."""
    n = keys.shape[0]
    empty = emu.hostemu_keyset_map_empty()
    m = Map(emu, keys)
    try:
        assert m.slots >= 4 * n and m.slots & (m.slots - 1) == 0
        assert 1 <= m.longest <= emu.hostemu_keyset_map_bound()
        exp, first = first_index(keys)
        assert np.array_equal(m.probe(keys), exp)
        flipped = keys.copy()
        flipped[np.arange(n), rng.integers(0, 32, n)] ^= (1 << rng.integers(0, 8, n)).astype(np.uint8)
        strangers = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
        for other in (flipped, strangers):
            want = np.array([first.get(k.tobytes(), empty) for k in other], np.uint32)
            got = m.probe(other)
            assert np.array_equal(got, want)
            assert (got == empty).sum() >= other.shape[0] - 1  # none of them is a member, bar a freak
        return m.slots, m.longest, m.seed
    finally:
        m.close()


@pytest.mark.parametrize("nkeys", NKEYS)
def test_random_sets(emu, nkeys):
    rng = np.random.default_rng(0xA11CE + nkeys)
    keys = rng.integers(0, 256, (nkeys, 32), dtype=np.uint8)
    for i in range(9, nkeys, 10):  # 10 % duplicates of an earlier key
        keys[i] = keys[rng.integers(0, i)]
    if nkeys >= 255:
        assert len({k.tobytes() for k in keys}) < nkeys
    slots, longest, seed = check_set(emu, keys, rng)
    assert slots == max(4, 1 << (4 * nkeys - 1).bit_length())
    assert seed == 0  # random keys: the first seed keeps the bound


def test_colliding_set_gets_a_later_seed(emu):
    """64 keys (256 slots), 40 of them with one home slot under seed 0 -- a
    probe sequence of 40 there, past the bound."""
    rng = np.random.default_rng(0xBAD5EED)
    bound = emu.hostemu_keyset_map_bound()
    assert bound < 40
    keys = []
    while len(keys) < 40:
        cand = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
        for k in cand:
            if emu.hostemu_keyset_map_hash(k.ctypes.data_as(ctypes.c_void_p), 0) & 255 == 201 and len(keys) < 40:
                keys.append(k.copy())
    keys = np.stack(keys + list(rng.integers(0, 256, (24, 32), dtype=np.uint8)))
    assert keys.shape == (64, 32)
    slots, longest, seed = check_set(emu, keys, rng)
    assert slots == 256 and seed > 0 and longest <= bound


def test_hash_uses_every_word_and_the_seed(emu):
    rng = np.random.default_rng(5)
    k = rng.integers(0, 256, 32, dtype=np.uint8)
    h = lambda key, seed: emu.hostemu_keyset_map_hash(key.ctypes.data_as(ctypes.c_void_p), seed)  # noqa: E731
    base = h(k, 0)
    for w in range(8):
        k2 = k.copy()
        k2[4 * w] ^= 1
        assert h(k2, 0) != base, w
    assert h(k, 1) != base and h(k, 1 << 32) != base and h(k, 1 << 63) != base


def test_sanitized_program():
    """tests/native/keyset_map_sanitize_main.cpp under ASan + UBSan, as a child
    process: the cases above from a generator of its own."""
    out = os.path.join(NATIVE, "san")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "keyset_map_sanitize_main")
    srcs = [os.path.join(NATIVE, f) for f in ("keyset_map_sanitize_main.cpp", "hostemu_keyset_map.cpp")]
    deps = srcs + [os.path.join(ROOT, "stellard_amd", "csrc", "stl_keyset_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-fno-gpu-sanitize", "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe, srcs[0]], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("failed checks 0")


# ---- the C ABI without a GPU ----
def test_by_key_argument_checks():
    """Argument errors come before any device work, on every machine."""
    from stellard_amd import _native as N
    lib = N.load()
    assert N.STL_KEYSET_NOT_FOUND == 0xFFFFFFFF
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    live = ctypes.c_void_p(8)  # not a live handle
    miss = ctypes.c_size_t(7)
    bm = ctypes.create_string_buffer(8)
    assert lib.stl_keyset_lookup_device(None, p, 1, p, None, None) == N.STL_EINVAL
    assert lib.stl_keyset_lookup_device(live, p, 1, p, None, None) == N.STL_EINVAL
    assert lib.stl_keyset_lookup_device(live, None, 1, p, None, None) == N.STL_EINVAL
    assert lib.stl_keyset_verify_by_key_device(None, p, p, p, 1, p, 0, None, ctypes.byref(miss)) == N.STL_EINVAL
    assert miss.value == 0
    assert lib.stl_keyset_verify_by_key(None, p, p, p, 1, bm, 0) == N.STL_EINVAL
    assert lib.stl_keyset_signed_blob_verify_batch_device(None, 0, p, p, p, 1, p, p, None, 0, None, None) == N.STL_EINVAL
    assert lib.stl_keyset_signed_blob_verify_batch_device(live, 7, p, p, p, 1, p, p, None, 0, None, None) == N.STL_EINVAL
    for flags in (0x40, N.STL_DEDUP_KEYS, N.STL_FULL_LENGTH, N.STL_ONE_LANE, N.STL_NO_AUTO_DEDUP):
        assert lib.stl_keyset_verify_by_key_device(live, p, p, p, 1, p, flags, None, None) == N.STL_EINVAL
        assert lib.stl_keyset_verify_by_key(live, p, p, p, 1, bm, flags) == N.STL_EINVAL
        assert lib.stl_keyset_signed_blob_verify_batch_device(live, 1, p, p, p, 1, p, p, None, flags, None,
                                                              None) == N.STL_EINVAL
    # a handle that is not live, with good arguments otherwise
    assert lib.stl_keyset_verify_by_key_device(live, p, p, p, 1, p, 0, None, None) == N.STL_EINVAL
    assert lib.stl_keyset_verify_by_key(live, p, p, p, 1, bm, 0) == N.STL_EINVAL
