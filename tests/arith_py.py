"""Plain Python-integer reference for the arithmetic op table
(stellard_amd/csrc/stl_selftest.h): the value of a limb vector is
sum(v[i] << 29*i), the field is p = 2^255 - 19, scalars are mod L, points go
through tests/golden/ed25519_py.py, and lattice_half is compared with
tests/test_halfscalar.py::_lattice_euclid.

check(name, row_in, row_out) asserts, for one row, that the output VALUE is
right and that every output limb is within the bound the headers state for
that op.  Test infrastructure: never imported by the product package.
"""
import os
import re

from tests.golden import ed25519_py as ed
from tests.test_halfscalar import _lattice_euclid

P = ed.P
L = ed.L
M29 = (1 << 29) - 1
IN_WORDS, OUT_WORDS, FLAG = 72, 40, 36

# limb bounds the headers state (stl_fe25519.h, "limb-bound discipline")
MUL_OUT = (1 << 29) + (1 << 17)      # fe_mul / fe_sq family: alpha <= 1 + 2^-12
CARRY_OUT = (1 << 29) + (1 << 14)    # fe_carry / fe_sub:     alpha <= 1 + 2^-15
NEG_OUT = (1 << 29) + (1 << 13)      # fe_neg, fe_sub with limb 8 of a below 3*2^29: 1 + 2^-16
Z1 = [M29 - 1215] + [M29] * 8        # 2^261 - 1216 == 0 (mod p)
Z1_4 = [0x7fffed00] + [0x7ffffffc] * 8
SUB_CAP = 39 * (1 << 29) // 10       # floor(3.9 * 2^29)
MUL_CAP = 7 << 58                    # max limb of a  *  max limb of b

assert sum(z << (29 * i) for i, z in enumerate(Z1)) % P == 0
assert Z1_4 == [4 * z for z in Z1]


def _op_table():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stellard_amd", "csrc",
                       "stl_selftest.h")
    with open(src) as f:
        text = f.read()
    ops = re.findall(r"\b(kOp\w+)\b", text[text.index("enum SelftestOp"):text.index("kSelftestOps\n")])
    grp = re.findall(r"\b(kGrp\w+)\b", text[text.index("enum SelftestGroupOp"):text.index("kSelftestGroupOps\n")])
    return {n: i for i, n in enumerate(ops)}, {n: i for i, n in enumerate(grp)}


OPS, GROUP_OPS = _op_table()


def value(limbs):
    return sum(int(v) << (29 * i) for i, v in enumerate(limbs))


def to_limbs(x):
    """29-bit limbs of 0 <= x < 2^261 + (limb 8 takes what is left)."""
    assert x >= 0
    out = [(x >> (29 * i)) & M29 for i in range(8)]
    out.append(x >> 232)
    assert out[8] < 1 << 32
    return out


def words(x, n):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def unwords(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def fe(row, slot):
    return [int(v) for v in row[9 * slot:9 * slot + 9]]


def alpha_max(limbs):
    return max(limbs)


def _signed(v, bits):
    return v - (1 << bits) if v >> (bits - 1) else v


def digits(packed, bits, count):
    """count signed digits of `bits` bits, two's complement, LSB first."""
    x = unwords(packed)
    return [_signed((x >> (bits * i)) & ((1 << bits) - 1), bits) for i in range(count)]


def _eq_mod_p(got, exp, what):
    assert (value(got) - exp) % P == 0, (what, got, exp % P)


def _within(limbs, bound, what):
    assert max(limbs) <= bound, (what, [hex(v) for v in limbs], hex(bound))


def _zero_rest(o, used_words, flags=0):
    """every word an op does not write is 0"""
    assert not any(o[used_words:FLAG]), ("stray output words", list(o))
    assert not any(o[FLAG + flags:]), ("stray flag words", list(o))


def _p1p1_is(o, pt, what):
    """p1p1 ((X:Z),(Y:T)) equals the affine point of pt"""
    x, y = ed.affine(pt)
    X, Y, Z, T = (value(fe(o, j)) % P for j in range(4))
    assert Z != 0 and T != 0, what
    assert (X - x * Z) % P == 0 and (Y - y * T) % P == 0, what


def _pt_p3(row, slot=0):
    X, Y, Z, T = (value(fe(row, slot + j)) % P for j in range(4))
    return (X, Y, Z, T)


def _pt_cached(row, slot):
    ypx, ymx, Z, t2d = (value(fe(row, slot + j)) % P for j in range(4))
    inv2 = ed.inv(2)
    X, Y = (ypx - ymx) * inv2 % P, (ypx + ymx) * inv2 % P
    T = t2d * ed.inv(2 * ed.D) % P
    return (X, Y, Z, T)


def _pt_niels(row, slot):
    ypx, ymx, xy2d = (value(fe(row, slot + j)) % P for j in range(3))
    inv2 = ed.inv(2)
    x, y = (ypx - ymx) * inv2 % P, (ypx + ymx) * inv2 % P
    assert (xy2d - 2 * ed.D * x * y) % P == 0
    return (x, y, 1, x * y % P)


def _add_bounds(o, what):
    # X = B + 2 Z1 - A [3], Y = B + A [2], Z = D + C [3], T fe_sub
    _within(fe(o, 0), MUL_OUT + 2 * M29, what + " X")
    _within(fe(o, 1), 2 * MUL_OUT, what + " Y")
    _within(fe(o, 2), 3 * MUL_OUT, what + " Z")
    _within(fe(o, 3), NEG_OUT, what + " T")  # a = D [2]: limb 8 of a below 3*2^29


def check(name, r, o):  # noqa: C901 - one branch per op of the table
    r = [int(v) for v in r]
    o = [int(v) for v in o]
    f = [fe(r, j) for j in range(8)]
    v = [value(x) for x in f]
    g = [fe(o, j) for j in range(4)]
    flag = o[FLAG:]
    if name in ("kOpFeMul", "kOpFeMul2", "kOpFeMul3", "kOpFeMul4"):
        n = {"kOpFeMul": 1, "kOpFeMul2": 2, "kOpFeMul3": 3, "kOpFeMul4": 4}[name]
        for j in range(n):
            _eq_mod_p(g[j], v[2 * j] * v[2 * j + 1], (name, j))
            _within(g[j], MUL_OUT, (name, j))
        _zero_rest(o, 9 * n)
    elif name in ("kOpFeSq", "kOpFeSq2", "kOpFeSqN3", "kOpFeSq4"):
        n = {"kOpFeSq": 1, "kOpFeSq2": 2, "kOpFeSqN3": 3, "kOpFeSq4": 4}[name]
        for j in range(n):
            _eq_mod_p(g[j], v[j] * v[j], (name, j))
            _within(g[j], MUL_OUT, (name, j))
        _zero_rest(o, 9 * n)
    elif name == "kOpFeSqn":
        n = r[9] & 63
        _eq_mod_p(g[0], pow(v[0], 1 << max(n, 1), P), name)
        _within(g[0], MUL_OUT, name)
        _zero_rest(o, 9)
    elif name == "kOpFeAdd":
        assert g[0] == [a + b for a, b in zip(f[0], f[1])], name  # no carry: limb sums
        _zero_rest(o, 9)
    elif name == "kOpFeSub":
        _eq_mod_p(g[0], v[0] - v[1], name)
        _within(g[0], CARRY_OUT, name)
        if f[0][8] < 3 << 29:
            _within(g[0], NEG_OUT, name + " (limb 8 of a below 3*2^29)")
        _zero_rest(o, 9)
    elif name == "kOpFeNeg":
        _eq_mod_p(g[0], -v[0], name)
        _within(g[0], NEG_OUT, name)
        _zero_rest(o, 9)
    elif name in ("kOpFeSubNc2", "kOpFeSubNc3"):
        k = 2 if name == "kOpFeSubNc2" else 3
        assert g[0] == [a + k * z - b for a, z, b in zip(f[0], Z1, f[1])], name
        _eq_mod_p(g[0], v[0] - v[1], name)
        _within(g[0], max(f[0]) + k * M29, name)  # alpha <= alpha_a + K
        _zero_rest(o, 9)
    elif name == "kOpFeNegNc2":
        assert g[0] == [2 * z - a for z, a in zip(Z1, f[0])], name
        _eq_mod_p(g[0], -v[0], name)
        _zero_rest(o, 9)
    elif name == "kOpFeCarry":
        _eq_mod_p(g[0], v[0], name)
        _within(g[0], CARRY_OUT, name)
        _zero_rest(o, 9)
    elif name == "kOpFeCmov":
        assert g[0] == (f[1] if r[18] else f[0]), name
        _zero_rest(o, 9)
    elif name == "kOpFeFrombytes":
        x = unwords(r[:8]) & ((1 << 255) - 1)
        assert g[0] == to_limbs(x), name  # exact limbs, bit 255 ignored, no reduction
        _zero_rest(o, 9)
    elif name == "kOpFeTobytes":
        assert unwords(o[:8]) == v[0] % P, (name, f[0])
        _zero_rest(o, 8)
    elif name == "kOpFeIszero":
        assert flag[0] == (1 if v[0] % P == 0 else 0), (name, f[0])
        _zero_rest(o, 0, 1)
    elif name == "kOpFeIsnegative":
        assert flag[0] == (v[0] % P) & 1, (name, f[0])
        _zero_rest(o, 0, 1)
    elif name == "kOpFeInvert":
        _eq_mod_p(g[0], pow(v[0], P - 2, P), name)
        _within(g[0], MUL_OUT, name)
        _zero_rest(o, 9)
    elif name == "kOpFePow22523":
        _eq_mod_p(g[0], pow(v[0], (P - 5) // 8, P), name)
        _within(g[0], MUL_OUT, name)
        _zero_rest(o, 9)
    elif name in ("kOpFeConstD", "kOpFeConst2d", "kOpFeConstSqrtm1"):
        exp = {"kOpFeConstD": ed.D, "kOpFeConst2d": 2 * ed.D % P, "kOpFeConstSqrtm1": ed.SQRTM1}[name]
        assert g[0] == to_limbs(exp), name  # canonical limbs
        _zero_rest(o, 9)
    elif name == "kOpScReduce64":
        assert unwords(o[:8]) == unwords(r[:16]) % L, name
        _zero_rest(o, 8)
    elif name == "kOpScMuladd":
        assert unwords(o[:8]) == (unwords(r[:8]) * unwords(r[8:16]) + unwords(r[16:24])) % L, name
        _zero_rest(o, 8)
    elif name == "kOpScLtL":
        assert flag[0] == (1 if unwords(r[:8]) < L else 0), (name, hex(unwords(r[:8])))
        _zero_rest(o, 0, 1)
    elif name == "kOpScRecode16":
        d = digits(o[:8], 4, 64)
        assert sum(e << (4 * i) for i, e in enumerate(d)) == unwords(r[:8]), name
        assert all(-8 <= e <= 7 for e in d[:63]) and 0 <= d[63] <= 2, (name, d)
        _zero_rest(o, 8)
    elif name == "kOpScRecode256":
        d = digits(o[:8], 8, 32)
        assert sum(e << (8 * i) for i, e in enumerate(d)) == unwords(r[:8]), name
        assert all(-128 <= e <= 127 for e in d[:31]) and 0 <= d[31] <= 32, (name, d)
        _zero_rest(o, 8)
    elif name == "kOpScRecode65536":
        d = digits(o[:8], 16, 16)
        assert sum(e << (16 * i) for i, e in enumerate(d)) == unwords(r[:8]), name
        assert all(-32768 <= e <= 32767 for e in d[:15]) and 0 <= d[15] <= 1 << 13, (name, d)
        _zero_rest(o, 8)
    elif name == "kOpScMulSigned":
        d = unwords(r[:5]) * (-1 if r[5] else 1)
        assert unwords(o[:8]) == d * unwords(r[8:16]) % L, name
        _zero_rest(o, 8)
    elif name == "kOpLatticeHalf":
        check_lattice(r, o)
    elif name == "kOpScRecode16Half":
        d = digits(o[:5], 4, 40)
        assert sum(e << (4 * i) for i, e in enumerate(d)) == unwords(r[:5]), name
        assert all(-8 <= e <= 7 for e in d), (name, d)
        need = max([i + 1 for i, e in enumerate(d) if e] + [1])
        assert flag[0] == need, (name, flag[0], need)
        _zero_rest(o, 5, 1)
    elif name in ("kOpGeP2Dbl", "kOpGeP2DblLazy", "kOpGeAffineDbl"):
        X, Y = v[0] % P, v[1] % P
        Z = 1 if name == "kOpGeAffineDbl" else v[2] % P
        pt = (X, Y, Z, X * Y * ed.inv(Z) % P)
        _p1p1_is(o, ed.add(pt, pt), name)
        # p1p1 of a doubling: X, T [1] (fe_sub), Y [2], Z [3]; the lazy X is A + 3 Z1 - Y [4]
        _within(g[0], MUL_OUT + 3 * M29 if name == "kOpGeP2DblLazy" else NEG_OUT, name + " X")
        _within(g[1], 2 * MUL_OUT, name + " Y")
        _within(g[2], MUL_OUT + 2 * M29, name + " Z")
        _within(g[3], NEG_OUT, name + " T")
    elif name == "kOpGeAddCached":
        _p1p1_is(o, ed.add(_pt_p3(r), _pt_cached(r, 4)), name)
        _add_bounds(o, name)
    elif name == "kOpGeMadd":
        _p1p1_is(o, ed.add(_pt_p3(r), _pt_niels(r, 4)), name)
        _add_bounds(o, name)
    elif name in ("kOpGeP1p1ToP2", "kOpGeP1p1ToP3"):
        X, Y, Z, T = (x % P for x in v[:4])
        _eq_mod_p(g[0], X * T, name + " X")
        _eq_mod_p(g[1], Y * Z, name + " Y")
        _eq_mod_p(g[2], Z * T, name + " Z")
        n = 3
        if name == "kOpGeP1p1ToP3":
            _eq_mod_p(g[3], X * Y, name + " T")
            n = 4
        for j in range(n):
            _within(g[j], MUL_OUT, name)
        _zero_rest(o, 9 * n)
        if Z and T:  # as affine points: (X/Z, Y/T) before, (X/Z, Y/Z) after
            zi = ed.inv(value(g[2]) % P)
            assert (value(g[0]) * zi - X * ed.inv(Z)) % P == 0 and (value(g[1]) * zi - Y * ed.inv(T)) % P == 0, name
    elif name == "kOpGeP3ToCached":
        X, Y, Z, T = (x % P for x in v[:4])
        _eq_mod_p(g[0], Y + X, name + " YpX")
        _eq_mod_p(g[1], Y - X, name + " YmX")
        assert g[2] == f[2], name + " Z"
        _eq_mod_p(g[3], T * 2 * ed.D, name + " T2d")
        _within(g[0], NEG_OUT, name + " YpX")  # fe_carry of a [2] sum
        _within(g[1], NEG_OUT, name + " YmX")
        _within(g[3], MUL_OUT, name + " T2d")
    elif name == "kOpGeCachedCneg":
        neg = r[36] != 0
        nt = [2 * z - a for z, a in zip(Z1, f[3])]
        assert g == ([f[1], f[0], f[2], nt] if neg else f[:4]), name
        _eq_mod_p(g[3], -v[3] if neg else v[3], name)
    elif name == "kOpGeNielsCneg":
        neg = r[27] != 0
        nt = [2 * z - a for z, a in zip(Z1, f[2])]
        assert g[:3] == ([f[1], f[0], nt] if neg else f[:3]), name
        _zero_rest(o, 27)
    elif name == "kOpGeFrombytesNegate":
        s = unwords(r[:8]).to_bytes(32, "little")
        pt = ed.decode(s)
        assert flag[0] == (0 if pt is None else 1), (name, s.hex())
        for j in range(4):
            _within(g[j], MUL_OUT, name)
        if pt is not None:
            x, y = pt[0], pt[1]
            _eq_mod_p(g[0], -x, name + " X")
            _eq_mod_p(g[1], y, name + " Y")
            assert g[2] == [1] + [0] * 8, name + " Z"
            _eq_mod_p(g[3], -x * y, name + " T")
    elif name == "kOpGeTobytes":
        X, Y, Z = (x % P for x in v[:3])
        assert unwords(o[:8]).to_bytes(32, "little") == ed.encode((X, Y, Z, 0)), name
        _zero_rest(o, 8)
    else:
        raise KeyError(name)


def check_lattice(r, o):
    """(ok, c, d) of lattice_half equals the one-step-at-a-time Euclid's."""
    k = unwords(r[:8])
    ok = o[FLAG] != 0
    rok, rc, rd = _lattice_euclid(k)
    assert ok == bool(rok), ("lattice_half ok", hex(k), ok, rok)
    assert o[FLAG] in (0, 1) and o[FLAG + 1] in (0, 1) and o[FLAG + 2] in (0, 1)
    if ok:
        c = unwords(o[0:5]) * (-1 if o[FLAG + 1] else 1)
        d = unwords(o[5:10]) * (-1 if o[FLAG + 2] else 1)
        assert (c, d) == (rc, rd), ("lattice_half (c, d)", hex(k))
    assert not any(o[10:FLAG]) and not o[FLAG + 3]
