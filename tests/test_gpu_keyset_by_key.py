"""GPU tests of the keyset calls that take public keys (stl_keyset_lookup_device,
stl_keyset_verify_by_key*, stl_keyset_signed_blob_verify_batch_device): the
lookup answers as stl_keyset_find; a by-key verify gives the bits of the
per-signature call whatever part of the signers is registered; the closed-set,
host and blob forms; fault injection, concurrent streams and argument errors.

Run on an MI355X:  python -u -m pytest tests/test_gpu_keyset_by_key.py -m gpu -x -v
"""
import ctypes
import threading

import numpy as np
import pytest

from tests.test_keyset_host import keyset_of

pytestmark = pytest.mark.gpu

NOT_FOUND = 0xFFFFFFFF


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


def _cuda(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


class Rows:
    """n rows of test_gpu_keyset's recipe (five signers, about one row in three
    adversarial, the key-changing classes from a small parameter range), their
    distinct keys, and the per-signature call's bits -- computed once per n."""

    def __init__(self, stl, torch, n):
        rng = np.random.default_rng(0x5E75 + n)
        base = rng.integers(0, 256, (5, 32), np.uint8)
        seeds = base[np.arange(n) % 5]
        msgs = rng.integers(0, 256, (n, 32), np.uint8)
        self.cls = np.where(rng.random(n) < 1 / 3, 1 + rng.integers(0, 11, n), 0).astype(np.uint8)
        param = rng.integers(0, 32, n).astype(np.uint32)
        self.n = n
        self.pk, self.sig, self.msg = stl.sign_adversarial_device(*_cuda(torch, seeds, msgs, self.cls,
                                                                         param.view(np.int32)))
        self.hpk = self.pk.cpu().numpy()
        self.keys, self.idx = keyset_of(self.hpk)
        self.ref = {}
        for policy in (0, 1):
            words = stl.verify_batch_device(self.sig, self.msg, self.pk, policy=policy)
            torch.cuda.synchronize()
            self.ref[policy] = stl.words_to_bool(words, n)
        self._oracle = {}

    def oracle_bits(self, oracle, policy):
        if policy not in self._oracle:
            self._oracle[policy] = oracle.verify_batch(self.sig.cpu().numpy(), self.msg.cpu().numpy(), self.hpk,
                                                       policy=policy)
        return self._oracle[policy]


@pytest.fixture(scope="module")
def rows_of(stl, torch_cuda):
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = Rows(stl, torch_cuda, n)
        return cache[n]
    return get


STRANGER = np.frombuffer(bytes(range(100, 132)), np.uint8)  # a key no row is signed with


def registered(rows, fraction):
    """The distinct keys (first-appearance order) a case registers -> bool mask."""
    k = rows.keys.shape[0]
    m = np.ones(k, bool)
    if fraction == "none":
        m[:] = False
    elif fraction == "every_other":
        m[1::2] = False
    elif fraction == "all_but_first_row":
        m[rows.idx[0]] = False
    elif fraction == "all_but_last_row":
        m[rows.idx[-1]] = False
    else:
        assert fraction == "all"
    return m


def keyset_for(stl, rows, mask):
    keys = rows.keys[mask] if mask.any() else STRANGER.reshape(1, 32)
    return stl.Keyset(keys)


# ---- 1. lookup ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_lookup_equals_find(stl, torch_cuda, rows_of, n):
    torch = torch_cuda
    r = rows_of(n)
    mask = registered(r, "every_other")
    reg = r.keys[mask]
    # the set with every third key registered a second time, further back: the first index answers
    dup = np.concatenate([reg, reg[::3]])
    with stl.Keyset(dup) as ks:
        find = np.array([ks.find(k.tobytes()) for k in r.keys], np.int64)
        assert ((find >= 0) == mask).all() and (find < reg.shape[0]).all()
        exp = np.where(find < 0, NOT_FOUND, find).astype(np.uint32)[r.idx]
        count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        got = ks.lookup_device(r.pk, miss_count=count)
        plain = ks.lookup_device(r.pk)  # without the counter
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), exp)
        assert np.array_equal(plain.cpu().numpy().view(np.uint32), exp)
        assert int(count.item()) == int((exp == NOT_FOUND).sum())


def test_lookup_in_a_full_set(stl, torch_cuda):
    """4,096 keys (the largest set: 16,384 slots), 4,099 rows of members,
    duplicates and strangers."""
    from stellard_amd import _native as N
    torch = torch_cuda
    rng = np.random.default_rng(4096)
    keys = rng.integers(0, 256, (N.STL_KEYSET_MAX_KEYS, 32), dtype=np.uint8)
    keys[1000] = keys[3]
    keys[4095] = keys[4000]
    n = 4099
    pick = rng.integers(0, keys.shape[0], n)
    pick[:4] = [1000, 4095, 0, 4094]
    pk = keys[pick].copy()
    strangers = rng.random(n) < 0.25
    strangers[:4] = False
    pk[strangers] = rng.integers(0, 256, (int(strangers.sum()), 32), dtype=np.uint8)
    exp = pick.astype(np.uint32)
    exp[pick == 1000] = 3
    exp[pick == 4095] = 4000
    exp[strangers] = NOT_FOUND
    with stl.Keyset(keys) as ks:
        assert ks.find(keys[1000].tobytes()) == 3 and ks.find(keys[4095].tobytes()) == 4000
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = ks.lookup_device(_cuda(torch, pk)[0], miss_count=count)
        torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), exp)
    assert int(count.item()) == int(strangers.sum()) > 900


# ---- 2. the bits of the per-signature call, whatever is registered ----
# Edges: the 64-lane wave (63 / 64 / 65) and the 256-lane workgroup (255 / 256 /
# 257) of the lookup, gather and scatter kernels; 70,001 is past 65,536.
SIZES = [1, 63, 64, 65, 255, 256, 257, 4099, 70001]
FRACTIONS = ["none", "all", "every_other", "all_but_first_row", "all_but_last_row"]


@pytest.mark.parametrize("fraction", FRACTIONS)
@pytest.mark.parametrize("n", SIZES)
def test_same_bits_as_per_signature_call(stl, torch_cuda, oracle, rows_of, n, fraction):
    torch = torch_cuda
    r = rows_of(n)
    mask = registered(r, fraction)
    miss_rows = ~mask[r.idx]
    with keyset_for(stl, r, mask) as ks:
        for policy in (0, 1):
            words, misses = ks.verify_by_key_device(r.pk, r.sig, r.msg, policy=policy)
            torch.cuda.synchronize()
            got, exp = stl.words_to_bool(words, n), r.ref[policy]
            assert misses == int(miss_rows.sum()), (n, fraction, policy)
            assert np.array_equal(got, exp), (n, fraction, policy, np.nonzero(got != exp)[0][:10])
            assert got[r.cls == 0].all()
            if n <= 4099:
                assert np.array_equal(got, r.oracle_bits(oracle, policy))
            if n >= 255 and fraction == "every_other":
                # accepts and rejects among the hits and among the misses
                for part in (miss_rows, ~miss_rows):
                    assert got[part].any() and not got[part].all(), (n, policy)
    if fraction == "none":
        assert miss_rows.all()
    if fraction == "all":
        assert not miss_rows.any()
    if fraction == "all_but_first_row":
        assert miss_rows[0]
    if fraction == "all_but_last_row":
        assert miss_rows[-1]


# ---- 3. closed-set form ----
@pytest.mark.parametrize("n", [65, 4099])
def test_lookup_then_indexed_verify_is_the_closed_set_check(stl, torch_cuda, rows_of, n):
    torch = torch_cuda
    r = rows_of(n)
    mask = registered(r, "every_other")
    miss_rows = ~mask[r.idx]
    assert miss_rows.any() and not miss_rows.all()
    with keyset_for(stl, r, mask) as ks:
        for policy in (0, 1):
            idx = ks.lookup_device(r.pk)
            words = ks.verify_batch_device(idx, r.sig, r.msg, policy=policy)  # same stream: no wait in between
            torch.cuda.synchronize()
            exp = r.ref[policy].copy()
            exp[miss_rows] = False
            assert np.array_equal(stl.words_to_bool(words, n), exp), policy


# ---- 4. host form, stats ----
def test_host_form_and_stats(stl, torch_cuda, rows_of):
    torch = torch_cuda
    r = rows_of(4099)
    mask = registered(r, "every_other")
    with keyset_for(stl, r, mask) as ks:
        words, misses = ks.verify_by_key_device(r.pk, r.sig, r.msg)
        torch.cuda.synchronize()
        dev = stl.words_to_bool(words, r.n)
        assert 0 < misses < r.n
        stl.reset_stats()
        host = ks.verify_by_key(r.hpk, r.sig.cpu().numpy(), r.msg.cpu().numpy())
        st = stl.get_stats()
    assert np.array_equal(host, dev) and np.array_equal(host, r.ref[0])
    # each row once: the misses are not counted again by the per-signature kernels
    assert st["signatures"] == r.n and st["batches"] == 1 and st["accepted"] == int(dev.sum())


# ---- 5. blob form ----
def test_blob_form_equals_the_per_signature_blob_call(stl, torch_cuda, oracle):
    """The 600 validations + 4 transactions of test_validations_vs_oracle, 4 of
    the 6 validators registered."""
    from stellard_amd.verify import _pack
    from tests import txblob
    torch = torch_cuda
    rng = np.random.default_rng(51)
    keys = [oracle.keypair(rng.bytes(32)) for _ in range(6)]
    blobs = []
    for i in range(600):
        pk, sk = keys[i % 6]
        fs = txblob.validation_fields(rng, pk, full=bool(i % 2))
        b, _, _ = txblob.signed_validation(fs, sk, oracle.sign)
        x = rng.random()
        if x < 0.15:
            b = bytearray(b)
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
            b = bytes(b)
        elif x < 0.2:
            b = b[: int(rng.integers(1, len(b)))]  # truncated
        blobs.append(b)
    blobs += txblob.valid_corpus(oracle, 4, 52)
    n = len(blobs)
    exp, exp_ids = oracle.signed_blob_verify_batch(1, blobs, ids=True)
    buf, offs, lens = _pack(blobs)
    dbuf, doff, dlen = _cuda(torch, buf, offs.view(np.int64), lens.view(np.int32))
    reg = np.frombuffer(b"".join(bytes(keys[j][0]) for j in (0, 1, 3, 4)), np.uint8).reshape(4, 32)
    outs = []
    with stl.Keyset(reg) as ks:
        for call in (stl.signed_blob_verify_batch_device, ks.signed_blob_verify_batch_device):
            status = torch.zeros(n, dtype=torch.uint8, device="cuda")
            ids = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
            o = call(dbuf, doff, dlen, kind=stl.BLOB_VALIDATION, out_status=status, out_ids=ids)
            torch.cuda.synchronize()
            outs.append((stl.words_to_bool(o["words"], n), status.cpu().numpy(), ids.cpu().numpy(), o))
    (ref_bits, ref_status, ref_ids, _), (bits, status, ids, o) = outs
    assert np.array_equal(bits, ref_bits) and np.array_equal(bits, exp)
    assert np.array_equal(status, ref_status) and np.array_equal(ids, ref_ids)
    dec = status != stl.TX_DEFERRED
    assert dec[:600].sum() > 450 and np.array_equal(ids[dec], exp_ids[dec])
    assert exp[:600].sum() > 400 and not bits[600:].any()
    # two of the six validators are not registered: about a third of the rows
    assert 150 < o["misses"] < 300


# ---- 6. fault injection ----
def test_fault_injection(stl, torch_cuda, rows_of):
    """Every HIP call of one by-key call on a batch with misses, failed in
    turn: the call returns < 0, and the same keyset then gives the right bits."""
    from stellard_amd import _native as N
    torch = torch_cuda
    r = rows_of(257)
    mask = registered(r, "every_other")
    n_miss = int((~mask[r.idx]).sum())
    assert 0 < n_miss < r.n
    stream = torch.cuda.Stream()  # a fresh context: the first calls also allocate
    failed, k = 0, 0
    with keyset_for(stl, r, mask) as ks, torch.cuda.stream(stream):
        try:
            while True:
                assert k < 96, "the countdown never ran out"
                stl.debug_fault_after(k)
                k += 1
                try:
                    words, misses = ks.verify_by_key_device(r.pk, r.sig, r.msg)
                except N.StlError as e:
                    assert e.rc < 0
                    failed += 1
                    stl.debug_fault_after(-1)
                    torch.cuda.synchronize()
                    good, m = ks.verify_by_key_device(r.pk, r.sig, r.msg)
                    torch.cuda.synchronize()
                    assert m == n_miss and np.array_equal(stl.words_to_bool(good, r.n), r.ref[0]), k
                    continue
                torch.cuda.synchronize()
                assert misses == n_miss and np.array_equal(stl.words_to_bool(words, r.n), r.ref[0])
                break  # no call left to fail
        finally:
            stl.debug_fault_after(-1)
    torch.cuda.synchronize()
    # memset, lookup, copy, event, keyset verify, wait, gather, the per-signature launch, scatter
    assert failed == k - 1 and failed >= 9


# ---- 7. concurrency and errors ----
def test_two_streams_one_keyset(stl, torch_cuda, rows_of):
    torch = torch_cuda
    r = rows_of(4099)
    mask = registered(r, "every_other")
    n_miss = int((~mask[r.idx]).sum())
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, errs = [[], []], []
    torch.cuda.synchronize()
    with keyset_for(stl, r, mask) as ks:
        def worker(s):
            try:
                for rep in range(4):
                    outs[s].append(ks.verify_by_key_device(r.pk, r.sig, r.msg, policy=s, stream=streams[s]))
            except Exception as e:  # noqa: BLE001 - reported below
                errs.append(e)

        ts = [threading.Thread(target=worker, args=(s,)) for s in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        torch.cuda.synchronize()
    assert not errs, errs
    for s in range(2):
        assert len(outs[s]) == 4
        for words, misses in outs[s]:
            assert misses == n_miss
            assert np.array_equal(stl.words_to_bool(words, r.n), r.ref[s]), s


def test_destroyed_handle_and_bad_flag_are_einval(stl, torch_cuda, rows_of):
    from stellard_amd import _native as N
    torch = torch_cuda
    lib = N.load()
    r = rows_of(65)
    ks = keyset_for(stl, r, registered(r, "every_other"))
    h = ks.handle
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    idx = torch.zeros(65, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    miss = ctypes.c_size_t(0)
    args = (p(r.pk), p(r.sig), p(r.msg), r.n, p(out))
    assert lib.stl_keyset_verify_by_key_device(h, *args, 0, None, ctypes.byref(miss)) == N.STL_OK
    torch.cuda.synchronize()
    assert miss.value > 0 and np.array_equal(stl.words_to_bool(out, r.n), r.ref[0])
    assert lib.stl_keyset_verify_by_key_device(h, *args, 0x40, None, None) == N.STL_EINVAL
    assert lib.stl_keyset_verify_by_key_device(h, None, p(r.sig), p(r.msg), r.n, p(out), 0, None, None) == N.STL_EINVAL
    assert lib.stl_keyset_verify_by_key_device(h, *args[:3], 0, None, 0, None, None) == N.STL_OK  # n == 0
    assert lib.stl_keyset_lookup_device(h, p(r.pk), r.n, p(idx), None, None) == N.STL_OK
    torch.cuda.synchronize()
    ks.close()
    assert lib.stl_keyset_verify_by_key_device(h, *args, 0, None, None) == N.STL_EINVAL
    assert lib.stl_keyset_lookup_device(h, p(r.pk), r.n, p(idx), None, None) == N.STL_EINVAL
    bm = ctypes.create_string_buffer(16)
    assert lib.stl_keyset_verify_by_key(h, bytes(32 * 65), bytes(64 * 65), bytes(32 * 65), 65, bm, 0) == N.STL_EINVAL
    assert lib.stl_keyset_signed_blob_verify_batch_device(h, 1, p(r.pk), p(out), p(idx), 1, p(out), p(r.pk), None, 0,
                                                          None, None) == N.STL_EINVAL
