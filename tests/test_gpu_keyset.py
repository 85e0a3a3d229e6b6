"""GPU tests of the registered signer sets (stl_keyset_*, stl_keyset.hip):
the doubling-free verify from per-key comb tables gives the bits of the
per-signature kernels, the oracle and the golden file; the device tables are
word-identical to the host build of the same code; indices, bad keys, the
host and checkSign forms, fault injection and concurrent keysets.

Run on an MI355X:  python -u -m pytest tests/test_gpu_keyset.py -m gpu -x -v
"""
import ctypes

import numpy as np
import pytest

from tests.test_keyset_host import keyset_of, load_keyset_emu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def stl(torch_cuda):
    from stellard_amd import verify
    verify.init()
    return verify


@pytest.fixture(scope="module")
def emu():
    return load_keyset_emu()


def _cuda(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _ks_bits(stl, torch, ks, idx, sig, msg, policy=0):
    d = _cuda(torch, idx.view(np.int32), sig, msg)
    words = ks.verify_batch_device(*d, policy=policy)
    torch.cuda.synchronize()
    return stl.words_to_bool(words, sig.shape[0])


@pytest.fixture(scope="module")
def golden_ks(stl, golden):
    keys, idx = keyset_of(golden["pk"])
    ks = stl.Keyset(keys)
    yield ks, keys, idx
    ks.close()


# ---- 1. goldens ----
@pytest.mark.parametrize("policy,key", [(0, "expected_sodium_1_0_18"), (1, "expected_stellard_1_0_0_unpinned")])
def test_goldens(stl, torch_cuda, golden, golden_ks, policy, key):
    ks, keys, idx = golden_ks
    info = ks.info()
    assert info["nkeys"] == 525 == keys.shape[0]
    per_key = info["windows"] * info["rows_per_window"] * info["row_bytes"]
    assert info["table_bytes"] == (info["nkeys"] + 1) * per_key
    assert ks.find(keys[7].tobytes()) == 7 and ks.find(bytes(range(32))) == -1
    got = _ks_bits(stl, torch_cuda, ks, idx, golden["sig"], golden["msg"], policy)
    exp = golden[key].astype(bool)
    if policy == 0:
        assert int(exp.sum()) == 1060
    for c in range(len(golden["class_names"])):
        m = golden["cls"] == c
        assert int(got[m].sum()) == int(exp[m].sum()), str(golden["class_names"][c])
    assert np.array_equal(got, exp)


# ---- 2. repeated signers: the bits of verify_batch_device ----
# The keyset kernel has no chunk or grid edge (one launch, one lane per row):
# its edges are the 64-lane wave (63 / 64 / 65) and the 256-lane workgroup
# (255 / 256 / 257); 70,001 is past 65,536.
SIZES = [1, 63, 64, 65, 255, 256, 257, 4099, 70001]


@pytest.mark.parametrize("n", SIZES)
def test_same_bits_as_per_signature_call(stl, torch_cuda, oracle, n):
    torch = torch_cuda
    rng = np.random.default_rng(0x5E75 + n)
    base = rng.integers(0, 256, (5, 32), np.uint8)
    seeds = base[np.arange(n) % 5]
    msgs = rng.integers(0, 256, (n, 32), np.uint8)
    cls = np.where(rng.random(n) < 1 / 3, 1 + rng.integers(0, 11, n), 0).astype(np.uint8)
    # parameters from a small range: the key-changing classes then yield a few
    # hundred distinct keys at most, whatever n
    param = rng.integers(0, 32, n).astype(np.uint32)
    pk, sig, msg = stl.sign_adversarial_device(*_cuda(torch, seeds, msgs, cls, param.view(np.int32)))
    keys, idx = keyset_of(pk.cpu().numpy())
    assert keys.shape[0] <= 1024
    for policy in (0, 1):
        ref = stl.verify_batch_device(sig, msg, pk, policy=policy)
        with stl.Keyset(keys) as ks:
            words = ks.verify_batch_device(torch.from_numpy(idx.view(np.int32)).cuda(), sig, msg, policy=policy)
            torch.cuda.synchronize()
        got, exp = stl.words_to_bool(words, n), stl.words_to_bool(ref, n)
        assert np.array_equal(got, exp), (n, policy, np.nonzero(got != exp)[0][:10])
        assert got[cls == 0].all()
        if n <= 4099:
            assert np.array_equal(got, oracle.verify_batch(sig.cpu().numpy(), msg.cpu().numpy(), pk.cpu().numpy(),
                                                           policy=policy))
        if n >= 4099:
            assert got.any() and not got.all()


# ---- 3. device rows ----
def test_device_rows_equal_host_rows(stl, torch_cuda, golden, emu):
    from stellard_amd import _native as N
    names = [str(x) for x in golden["class_names"]]
    honest = golden["pk"][0].tobytes()
    mixed = golden["pk"][np.nonzero(golden["cls"] == names.index("B8_mixed_order_pk"))[0][0]].tobytes()
    keys = np.frombuffer(honest + mixed, np.uint8).reshape(2, 32)
    rng = np.random.default_rng(77)
    with stl.Keyset(keys) as ks:
        info = ks.info()
        R, W, words = info["rows_per_window"], info["windows"], info["row_bytes"] // 4
        for key, enc in ((0, honest), (1, mixed), (N.STL_KEYSET_BASE, None)):
            host = np.zeros((W * R, words), np.uint32)
            emu.hostemu_keyset_table(enc, host.ctypes.data_as(ctypes.c_void_p))
            assert host[:, :27].any() and not host[:, 27:].any()
            assert np.array_equal(ks.rows(key, 0, R), host[:R]), key                          # window 0
            assert np.array_equal(ks.rows(key, (W - 1) * R, R), host[(W - 1) * R:]), key      # the last window
            for r in rng.integers(0, W * R, 64):
                assert np.array_equal(ks.rows(key, int(r), 1)[0], host[r]), (key, int(r))
        with pytest.raises(N.StlError):
            ks.rows(2, 0, 1)
        with pytest.raises(N.StlError):
            ks.rows(0, W * R, 1)


# ---- 4. indices and bad keys ----
def test_bad_index(stl, torch_cuda, golden, golden_ks):
    from stellard_amd import _native as N
    ks, keys, idx = golden_ks
    rows = np.nonzero(golden["expected_sodium_1_0_18"])[0][:130]
    sig, msg = golden["sig"][rows], golden["msg"][rows]
    good = _ks_bits(stl, torch_cuda, ks, idx[rows], sig, msg)
    assert good.all()
    bad = idx[rows].copy()
    bad[[0, 64, 77, 129]] = [keys.shape[0], 0xFFFFFFFF, keys.shape[0] + 5, 1 << 31]
    got = _ks_bits(stl, torch_cuda, ks, bad, sig, msg)
    exp = good.copy()
    exp[[0, 64, 77, 129]] = False
    assert np.array_equal(got, exp)
    with pytest.raises(N.StlError) as e:
        ks.verify_batch(bad, sig, msg)
    assert e.value.rc == N.STL_EINVAL


def test_bad_keys_answer_as_the_per_signature_call(stl, torch_cuda, golden):
    names = [str(x) for x in golden["class_names"]]
    pick = []
    for c in ("B10_pk_not_on_curve", "B6_small_order_pk", "B9_noncanonical_pk", "B8_mixed_order_pk", "valid"):
        pick += list(np.nonzero(golden["cls"] == names.index(c))[0][:24])
    pick = np.array(pick)
    sig, msg, pk = golden["sig"][pick], golden["msg"][pick], golden["pk"][pick]
    keys, idx = keyset_of(pk)
    with stl.Keyset(keys) as ks:
        for policy in (0, 1):
            got = _ks_bits(stl, torch_cuda, ks, idx, sig, msg, policy)
            assert np.array_equal(got, stl.verify_batch(sig, msg, pk, policy=policy)), policy
            assert np.array_equal(ks.verify_batch(idx, sig, msg, policy=policy), got)


# ---- 5. host call, tx call, stats, faults, destroyed handles ----
def test_host_call_and_stats(stl, torch_cuda, golden, golden_ks):
    ks, keys, idx = golden_ks
    dev = _ks_bits(stl, torch_cuda, ks, idx, golden["sig"], golden["msg"])
    stl.reset_stats()
    host = ks.verify_batch(idx, golden["sig"], golden["msg"])
    assert np.array_equal(host, dev)
    st = stl.get_stats()
    assert st["accepted"] == int(dev.sum()) and st["signatures"] == dev.shape[0] and st["batches"] == 1


def test_tx_call_equals_hash_then_verify(stl, torch_cuda, oracle):
    torch = torch_cuda
    rng = np.random.default_rng(300)
    n = 300
    lens = rng.integers(76, 4097, n).astype(np.int32)
    lens[:2] = [76, 4096]
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    pre = rng.integers(0, 256, int(lens.astype(np.int64).sum()), np.uint8)
    base = rng.integers(0, 256, (7, 32), np.uint8)
    seeds = base[np.arange(n) % 7]
    dpre, doff, dlen, dseed = _cuda(torch, pre, offs, lens, seeds)
    msg = stl.tx_hash_batch_device(dpre, doff, dlen)
    pk, sig = stl.sign_batch_device(dseed, msg)
    sig[::5, 3] ^= 1  # every fifth signature broken
    keys, idx = keyset_of(pk.cpu().numpy())
    didx = torch.from_numpy(idx.view(np.int32)).cuda()
    with stl.Keyset(keys) as ks:
        two = ks.verify_batch_device(didx, sig, msg)
        one = ks.tx_verify_batch_device(didx, dpre, doff, dlen, sig)
        torch.cuda.synchronize()
    got = stl.words_to_bool(one, n)
    assert np.array_equal(got, stl.words_to_bool(two, n))
    exp = np.ones(n, bool)
    exp[::5] = False
    assert np.array_equal(got, exp)


def test_fault_injection(stl, torch_cuda, golden, golden_ks):
    """Every HIP call of a create plus one verify, failed in turn: the call
    returns < 0, never STL_OK with a bitmap; afterwards a keyset verifies the
    goldens as before."""
    from stellard_amd import _native as N
    torch = torch_cuda
    sel = np.arange(0, golden["sig"].shape[0], 8)
    sig, msg = golden["sig"][sel], golden["msg"][sel]
    keys, idx = keyset_of(golden["pk"][sel])
    exp = golden["expected_sodium_1_0_18"][sel].astype(bool)
    d = _cuda(torch, idx.view(np.int32), sig, msg)
    failed, k = 0, 0
    try:
        while True:
            assert k < 64, "the countdown never ran out"
            stl.debug_fault_after(k)
            k += 1
            try:
                ks = stl.Keyset(keys)
            except N.StlError as e:
                assert e.rc < 0
                failed += 1
                continue
            try:
                words = ks.verify_batch_device(*d)
            except N.StlError as e:
                assert e.rc < 0
                failed += 1
                stl.debug_fault_after(-1)
                # the same keyset still verifies
                assert np.array_equal(_ks_bits(stl, torch, ks, idx, sig, msg), exp)
                ks.close()
                continue
            torch.cuda.synchronize()
            assert np.array_equal(stl.words_to_bool(words, len(sel)), exp)
            ks.close()
            break  # no call left to fail
    finally:
        stl.debug_fault_after(-1)
    assert failed == k - 1 and failed >= 8
    with stl.Keyset(keys) as ks:  # a fresh one
        assert np.array_equal(_ks_bits(stl, torch, ks, idx, sig, msg), exp)
    ks, _, gidx = golden_ks  # and the one that lived through all of it: every golden vector
    assert np.array_equal(_ks_bits(stl, torch, ks, gidx, golden["sig"], golden["msg"]),
                          golden["expected_sodium_1_0_18"].astype(bool))


def test_destroyed_handle_is_einval(stl, torch_cuda, golden):
    from stellard_amd import _native as N
    lib = N.load()
    keys, idx = keyset_of(golden["pk"][:4])
    ks = stl.Keyset(keys)
    h = ks.handle
    d = _cuda(torch_cuda, idx.view(np.int32), golden["sig"][:4], golden["msg"][:4])
    out = torch_cuda.zeros(1, dtype=torch_cuda.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.stl_keyset_verify_batch_device(h, p(d[0]), p(d[1]), p(d[2]), 4, p(out), 0, None) == N.STL_OK
    torch_cuda.cuda.synchronize()
    assert lib.stl_keyset_verify_batch_device(h, p(d[0]), p(d[1]), p(d[2]), 4, p(out), 0x40, None) == N.STL_EINVAL
    ks.close()
    assert lib.stl_keyset_verify_batch_device(h, p(d[0]), p(d[1]), p(d[2]), 4, p(out), 0, None) == N.STL_EINVAL
    bm = ctypes.create_string_buffer(1)
    assert lib.stl_keyset_verify_batch(h, p(d[0]), bytes(256), bytes(128), 4, bm, 0) == N.STL_EINVAL
    assert lib.stl_keyset_find(h, bytes(32)) == -1
    lib.stl_keyset_destroy(h)  # ignored


# ---- 6. two keysets on two streams ----
def test_two_keysets_two_streams(stl, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(66)
    n = 3000
    sets = []
    for s in range(2):
        base = rng.integers(0, 256, (9 + s, 32), np.uint8)
        seeds = base[rng.integers(0, base.shape[0], n)]
        msgs = rng.integers(0, 256, (n, 32), np.uint8)
        dseed, dmsg = _cuda(torch, seeds, msgs)
        pk, sig = stl.sign_batch_device(dseed, dmsg)
        bad = rng.random(n) < 0.25
        sig[torch.from_numpy(np.nonzero(bad)[0]).cuda(), 40] ^= 4
        keys, idx = keyset_of(pk.cpu().numpy())
        sets.append((stl.Keyset(keys), torch.from_numpy(idx.view(np.int32)).cuda(), sig, dmsg, ~bad))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[], []]
    for rep in range(4):
        for s in range(2):
            ks, didx, sig, msg, _ = sets[s]
            outs[s].append(ks.verify_batch_device(didx, sig, msg, stream=streams[s]))
    torch.cuda.synchronize()
    for s in range(2):
        for w in outs[s]:
            assert np.array_equal(stl.words_to_bool(w, n), sets[s][4]), s
        sets[s][0].close()
