"""The gfx950 build of the field, scalar and group arithmetic, op by op
(stellard_amd/csrc/stl_selftest.hip through stl_debug_selftest_ops_device and
stl_debug_selftest_group_device) on the rows of tests/arith_cases.py.

The device compiles the same source as the host harness into a different
program -- fenced mad chains, scheduling barriers, x * rcp(y) for the Lehmer
quotient estimate, wave-wide votes in the Lehmer loops, DPP lane groups -- so
every output word must equal the host build's (tests/native/hostemu.cpp), which
tests/test_arith_ops_host.py holds against Python integers: integer arithmetic
does not depend on how it is scheduled, so the comparison has no tolerance.
lattice_half is also checked against the exact Euclid directly.
"""
import ctypes

import numpy as np
import pytest

from tests import arith_cases, arith_py as A, oracle_bind

pytestmark = pytest.mark.gpu

FILL = -1515870811  # 0xA5A5A5A5 as int32
PAD_ROWS = 8


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
    return oracle_bind.load_hostemu()


@pytest.fixture(scope="module")
def host(emu):
    """Host results per one-lane op, computed once on first use."""
    cache = {}

    def get(name):
        if name not in cache:
            out, viol = oracle_bind.hostemu_selftest_ops(emu, A.OPS[name], arith_cases.cases()[name])
            assert viol == 0
            out.setflags(write=False)
            cache[name] = out
        return cache[name]
    return get


def _launch(torch, records, call):
    """Runs call(out) on an output buffer of `records` records followed by
    PAD_ROWS more, all pre-filled with 0xA5 bytes; nothing past the last
    record may change.  Returns the records as uint32."""
    out = torch.full((records + PAD_ROWS, A.OUT_WORDS), FILL, dtype=torch.int32, device="cuda")
    call(out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[records:] == 0xA5A5A5A5).all(), "wrote past the last record"
    return got[:records]


def _device_ops(torch, stl, name, rows):
    d_rows = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    return _launch(torch, rows.shape[0], lambda out: stl.selftest_ops_device(A.OPS[name], d_rows, out=out))


def _same(name, rows, got, exp, what=""):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{name}{what}: {bad.size} of {rows.shape[0]} rows differ; row {i}: in "
                             f"{rows[i].tolist()} device {got[i].tolist()} host {exp[i].tolist()}")


def _take(a, n):
    """n rows of a, repeating from the start if a is shorter"""
    return a[np.arange(n) % a.shape[0]]


@pytest.mark.parametrize("name", sorted(A.OPS, key=A.OPS.get))
def test_op_equals_host(torch_cuda, stl, host, name):
    rows, exp = arith_cases.cases()[name], host(name)
    _same(name, rows, _device_ops(torch_cuda, stl, name, rows), exp)
    for n in (1, 63, 64, 65):  # a lone lane, a partial wave, a whole wave, one lane into the next
        r, e = _take(rows, n), _take(exp, n)
        _same(name, r, _device_ops(torch_cuda, stl, name, r), e, f" n={n}")


def test_lattice_half_equals_exact_euclid(torch_cuda, stl, host):
    """Lanes with different Lehmer round counts share a wave (every 64 rows
    hold a boundary or Fibonacci k next to random ones): (ok, c, d) equals
    the one-step-at-a-time Euclid's whatever a lane's neighbours are -- in
    row order, reversed, and with a partial last wave."""
    name = "kOpLatticeHalf"
    rows, exp = arith_cases.cases()[name], host(name)
    assert rows.shape[0] % 64 != 0
    whole = rows.shape[0] - rows.shape[0] % 64
    for what, idx in (("", np.arange(rows.shape[0])), (" reversed", np.arange(rows.shape[0])[::-1]),
                      (" whole waves", np.arange(whole)), (" n=63", np.arange(63)), (" n=65", np.arange(65)),
                      (" n=65 reversed", np.arange(whole - 65, whole)[::-1])):
        r = np.ascontiguousarray(rows[idx])
        got = _device_ops(torch_cuda, stl, name, r)
        if not what:  # the device's own words against the Euclid, once; the other orders against these
            for i in range(r.shape[0]):
                A.check_lattice([int(v) for v in r[i]], [int(v) for v in got[i]])
        _same(name, r, got, exp[idx], what)


GROUP_CASES = [(g, G) for g in sorted(A.GROUP_OPS, key=A.GROUP_OPS.get) for G in (2, 4)]


@pytest.mark.parametrize("gname,G", GROUP_CASES)
def test_group_op_equals_one_lane_formula(torch_cuda, stl, host, gname, G):
    """Every lane of a group holds the whole result, and it is the host's
    one-lane formula on the same row, limb for limb."""
    torch = torch_cuda
    name = arith_cases.GROUP_MAP[gname]
    rows, exp = arith_cases.cases()[name], host(name)
    if gname == "kGrpToP2":  # the first three outputs of the p3 conversion
        exp = exp.copy()
        exp[:, 27:] = 0
    for n in (rows.shape[0], 1, 15, 16, 17, 257):
        r, e = _take(rows, n), _take(exp, n)
        d_rows = torch.from_numpy(r.view(np.int32).copy()).cuda()
        got = _launch(torch, n * G, lambda out: stl.selftest_group_device(A.GROUP_OPS[gname], G, d_rows, out=out))
        got = got.reshape(n, G, A.OUT_WORDS)
        for j in range(1, G):
            bad = np.nonzero((got[:, j] != got[:, 0]).any(axis=1))[0]
            assert bad.size == 0, (f"{gname} G={G} n={n}: lane {j} of group {int(bad[0])} differs from lane 0: "
                                   f"{got[int(bad[0]), j].tolist()} vs {got[int(bad[0]), 0].tolist()}")
        _same(f"{gname} G={G}", r, got[:, 0], e, f" n={n}")


def test_bad_arguments(torch_cuda, stl):
    from stellard_amd import _native as N
    lib = N.load()
    buf = torch_cuda.zeros((4, N.STL_SELFTEST_IN_WORDS), dtype=torch_cuda.int32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    assert lib.stl_debug_selftest_ops_device(N.STL_SELFTEST_OPS, p, 1, p, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_ops_device(0, None, 1, p, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_ops_device(0, p, 1, None, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_group_device(N.STL_SELFTEST_GROUP_OPS, 4, p, 1, p, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_group_device(0, 3, p, 1, p, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_group_device(0, 2, None, 1, p, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_group_device(0, 2, p, 1, None, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_ops_device(0, p, 0, p, None) == N.STL_OK
    torch_cuda.cuda.synchronize()
    assert not buf.any()
