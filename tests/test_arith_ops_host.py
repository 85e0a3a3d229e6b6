"""Field, scalar and group arithmetic op by op on the host build of the device
source (tests/native/hostemu.cpp, hostemu_selftest_ops over the op table of
stellard_amd/csrc/stl_selftest.h) against Python integers (tests/arith_py.py)
on the rows of tests/arith_cases.py: limb patterns at the edge of each op's
documented precondition, boundary scalars, special points.

For every op: the output value is right, every output limb is within the
bound the header states, the bound hooks count no violation over the whole
generated set -- and the hooks are armed (a row just outside a precondition
raises the count).
"""
import ctypes

import numpy as np
import pytest

from tests import arith_cases, arith_py as A, oracle_bind


@pytest.fixture(scope="module")
def emu():
    return oracle_bind.load_hostemu()


@pytest.fixture(scope="module")
def host_results(emu):
    """{op: (results, violations)} of the whole generated set, computed once."""
    return {name: oracle_bind.hostemu_selftest_ops(emu, A.OPS[name], rows)
            for name, rows in arith_cases.cases().items()}


def test_op_table_matches_header():
    from stellard_amd import _native as N
    assert len(A.OPS) == N.STL_SELFTEST_OPS and len(A.GROUP_OPS) == N.STL_SELFTEST_GROUP_OPS
    assert (A.IN_WORDS, A.OUT_WORDS) == (N.STL_SELFTEST_IN_WORDS, N.STL_SELFTEST_OUT_WORDS)
    assert set(arith_cases.GROUP_MAP) == set(A.GROUP_OPS)
    assert set(arith_cases.cases()) == set(A.OPS)


@pytest.mark.parametrize("name", sorted(A.OPS, key=A.OPS.get))
def test_op_matches_reference(host_results, name):
    rows = arith_cases.cases()[name]
    out, viol = host_results[name]
    assert rows.shape[0] > 0
    for i in range(rows.shape[0]):
        try:
            A.check(name, rows[i], out[i])
        except AssertionError as e:
            raise AssertionError(f"{name} row {i}: in {rows[i].tolist()} out {out[i].tolist()}: {e}") from None
    assert viol == 0, f"{name}: {viol} limb-bound violations on rows inside the documented preconditions"


def test_no_bound_violation_over_the_whole_set(host_results):
    assert {n: v for n, (_, v) in host_results.items() if v} == {}


def test_fe_sub_limb0_carry_witness(emu):
    """fe_carry folds (limb 8 >> 29) * 1216 into limb 0; with limb 8 of
    a + 4 Z1 - b at 7 * 2^29 that is 8512 > 2^13, so fe_sub's output bound is
    alpha <= 1 + 2^-15, not 1 + 2^-16 (which holds while limb 8 of a stays
    below 3 * 2^29, as it does at every call site of the group formulas)."""
    a = [3 * (1 << 29) + 0x12ff, 0, 0, 0, 0, 0, 0, 0, 3 * (1 << 29) + 4]
    row = np.array([arith_cases._row([a, [0] * 9])], np.uint32)
    out, viol = oracle_bind.hostemu_selftest_ops(emu, A.OPS["kOpFeSub"], row)
    assert viol == 0
    got = A.fe(out[0], 0)
    assert got[0] == (1 << 29) + 8511
    assert A.NEG_OUT < got[0] <= A.CARRY_OUT
    A.check("kOpFeSub", row[0], out[0])


def _viol(emu, name, slots):
    row = np.array([arith_cases._row(slots)], np.uint32)
    return oracle_bind.hostemu_selftest_ops(emu, A.OPS[name], row)[1]


def test_mul_hook_is_armed(emu):
    """STL_BOUND_MUL's predicate (alpha_a * alpha_b > 7) fires just above 7
    and not at 7; each count is the difference across one call."""
    one = 1 << 29
    at = [[7 * one] * 9, [one] * 9]
    above = [[7 * one] * 9, [one + 1] * 9]
    assert _viol(emu, "kOpFeMul", at) == 0
    assert _viol(emu, "kOpFeMul", above) == 1
    assert _viol(emu, "kOpFeMul", [[7 * one + 1] + [0] * 8, [0] * 8 + [one]]) == 1  # the max over limbs
    assert _viol(emu, "kOpFeMul4", at * 3 + above) == 1
    assert _viol(emu, "kOpFeMul2", above + above) == 2
    s7 = arith_cases.SQRT7
    assert _viol(emu, "kOpFeSq", [[s7] * 9]) == 0
    assert _viol(emu, "kOpFeSq", [[s7 + 1] * 9]) == 1
    assert _viol(emu, "kOpFeSq4", [[s7] * 9] * 3 + [[s7 + 1] * 9]) == 1


def test_sub_hooks_are_armed(emu):
    cap = A.SUB_CAP
    assert _viol(emu, "kOpFeSub", [[cap] * 9, [cap] * 9]) == 0
    assert _viol(emu, "kOpFeSub", [[cap + 1] + [0] * 8, [0] * 9]) == 1
    assert _viol(emu, "kOpFeSub", [[0] * 9, [0] * 8 + [cap + 1]]) == 1
    z2 = [2 * z for z in A.Z1]
    amax = (1 << 32) - 1 - 2 * A.M29
    assert _viol(emu, "kOpFeSubNc2", [[amax] * 9, z2]) == 0
    assert _viol(emu, "kOpFeSubNc2", [[0] * 9, [z2[0] + 1] + z2[1:]]) == 1
    assert _viol(emu, "kOpFeSubNc2", [[amax + 1] + [0] * 8, [0] * 9]) == 1
    assert _viol(emu, "kOpFeSubNc3", [[0] * 9, [0] * 8 + [3 * A.M29 + 1]]) == 1


def test_unknown_op_is_refused(emu):
    out = np.zeros((1, A.OUT_WORDS), np.uint32)
    row = np.zeros((1, A.IN_WORDS), np.uint32)
    V = ctypes.c_void_p
    rc = emu.hostemu_selftest_ops(len(A.OPS), row.ctypes.data_as(V), 1, out.ctypes.data_as(V))
    assert rc == 2**64 - 1 and not out.any()


def test_device_entries_refuse_bad_arguments():
    """Argument checks come before any device work, so they answer on every
    box: a bad op, a bad G, too many rows or a null pointer is STL_EINVAL."""
    from stellard_amd import _native as N
    lib = N.load()
    buf = ctypes.create_string_buffer(4 * N.STL_SELFTEST_IN_WORDS * 4)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.stl_debug_selftest_ops_device(N.STL_SELFTEST_OPS, p, 1, p, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_ops_device(0, None, 1, p, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_ops_device(0, p, 1, None, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_ops_device(0, p, N.STL_SELFTEST_MAX_ROWS + 1, p, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_group_device(N.STL_SELFTEST_GROUP_OPS, 4, p, 1, p, None) == N.STL_EINVAL
    for g in (0, 1, 3, 8):
        assert lib.stl_debug_selftest_group_device(0, g, p, 1, p, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_group_device(0, 2, None, 1, p, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_group_device(0, 4, p, 1, None, None) == N.STL_EINVAL
    assert lib.stl_debug_selftest_group_device(0, 4, p, N.STL_SELFTEST_MAX_ROWS + 1, p, None) == N.STL_EINVAL
