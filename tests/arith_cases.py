"""Rows for the arithmetic op table (stellard_amd/csrc/stl_selftest.h), shared
by tests/test_arith_ops_host.py and tests/test_gpu_arith_ops.py.

cases() returns {op name: (n, 72) uint32 array}.  Every row meets the
precondition its op documents -- the generator asserts that on each row it
emits (limb caps are integers: math.isqrt and integer products, no floats) --
so no consumer filters, skips or special-cases a row.
"""
import functools
import math
import random

import numpy as np

from tests import arith_py as A
from tests.golden import ed25519_py as ed
from tests.test_halfscalar import _boundary_ks, _fib_ks

P, L, M29 = A.P, A.L, A.M29
ONE = 1 << 29
SQRT7 = math.isqrt(7 << 58)            # largest limb with limb^2 <= 7 * 2^58
MUL1 = A.MUL_OUT                       # [1] as a product leaves it
ADD3 = A.MUL_OUT + 2 * M29             # [3] = [1] + 2 Z1 (fe_sub_nc<2>)
ADD4 = A.MUL_OUT + 3 * M29             # [4] = [1] + 3 Z1 (the lazy TO_P2 X)

# cap pairs (largest limb of a, of b) with A * B <= 7 * 2^58: the header's edge,
# then the combinations the group formulas make (stl_ge25519.h): 3x1, 2x1, 2x3,
# 3x2, and 4x1 for the lazy TO_P2 X
MUL_CAPS = [(ONE - 1, ONE - 1), (MUL1, MUL1), (7 * ONE, ONE), (ONE, 7 * ONE), (3 * ONE, 2 * ONE), (SQRT7, SQRT7),
            (ADD3, MUL1), (2 * MUL1, MUL1), (2 * MUL1, ADD3), (ADD3, 2 * MUL1), (ADD4, A.CARRY_OUT)]
SQ_CAPS = [ONE - 1, 2 * ONE, SQRT7, 2 * MUL1]

SPECIAL = [0, 1, 2, P - 1, P, P + 1, 2 * P - 1, 2 * P, (1 << 255) - 1]


def _caps(cap):
    return [cap] * 9 if isinstance(cap, int) else list(cap)


def special_limbs():
    """canonical limbs of 0, 1, 2, p-1 and the limbs fe_frombytes makes of the
    non-canonical encodings p, p+1, 2p-1, 2p, 2^255-1 (bit 255 dropped)"""
    return [A.to_limbs(x & ((1 << 255) - 1)) for x in SPECIAL]


def patterns(cap, rng, nrand):
    """The limb patterns of one cap (an int, or nine per-limb caps)."""
    c = _caps(cap)
    out = [list(c), [0] * 9]
    out += [[c[i] if i == j else 0 for i in range(9)] for j in range(9)]
    out += [[c[i] if i % 2 == ph else 0 for i in range(9)] for ph in (0, 1)]
    out += [[max(c[i] - j, 0) for i in range(9)] for j in range(5)]
    out += [[max(c[i] - (i + s) % 5, 0) for i in range(9)] for s in range(2)]
    out += [[rng.randint(0, c[i]) for i in range(9)] for _ in range(nrand)]
    out += [s for s in special_limbs() if all(s[i] <= c[i] for i in range(9))]
    for p in out:
        assert all(0 <= p[i] <= c[i] for i in range(9))
    return out


def _row(slots=(), words=None, at=None):
    r = [0] * A.IN_WORDS
    for j, s in enumerate(slots):
        r[9 * j:9 * j + 9] = s
    if words is not None:
        r[:len(words)] = words
    for k, v in (at or {}).items():
        r[k] = v
    return r


def _arr(rows):
    a = np.array(rows, dtype=np.uint64)
    assert a.ndim == 2 and a.shape[1] == A.IN_WORDS and a.max() < 1 << 32
    return a.astype(np.uint32)


# ---- field --------------------------------------------------------------

def mul_pairs(rng):
    """(a, b) limb vectors for one product, every pair within a * b <= 7."""
    out = []
    for ca, cb in MUL_CAPS:
        assert ca * cb <= A.MUL_CAP
        pa, pb = patterns(ca, rng, 24), patterns(cb, rng, 24)
        n = len(pa)
        assert len(pb) == n
        for s in (0, 1, 5):
            out += [(pa[i], pb[(i + s) % n]) for i in range(n)]
        out += [(pa[0], pb[i]) for i in range(n)] + [(pa[i], pb[0]) for i in range(n)]
    for a, b in out:
        assert max(a) * max(b) <= A.MUL_CAP
    return out


def sq_inputs(rng):
    out = []
    for c in SQ_CAPS:
        assert c * c <= A.MUL_CAP
        out += patterns(c, rng, 40)
    return out


def _rotations(items, k, steps):
    """rows of k different items: item i with items i + steps[1], ..."""
    n = len(items)
    return [[items[(i + s) % n] for s in steps[:k]] for i in range(n)]


def field_cases(rng):
    c = {}
    mp = mul_pairs(rng)
    c["kOpFeMul"] = _arr([_row(p) for p in mp])
    # every slot of the interleaved forms gets another pattern (and cap pair)
    for name, k in (("kOpFeMul2", 2), ("kOpFeMul3", 3), ("kOpFeMul4", 4)):
        c[name] = _arr([_row([x for pr in grp for x in pr]) for grp in _rotations(mp, k, (0, 37, 101, 211))][::2])
    sq = sq_inputs(rng)
    c["kOpFeSq"] = _arr([_row([a]) for a in sq])
    for name, k in (("kOpFeSq2", 2), ("kOpFeSqN3", 3), ("kOpFeSq4", 4)):
        c[name] = _arr([_row(grp) for grp in _rotations(sq, k, (0, 29, 67, 113))])
    c["kOpFeSqn"] = _arr([_row([a], at={9: n}) for n in (1, 2, 5, 50) for a in sq[::2]])

    big = patterns((1 << 31) - 1, rng, 40)
    c["kOpFeAdd"] = _arr([_row([a, b]) for a, b in zip(big, big[7:] + big[:7])])

    sub = []
    for ca, cb in ((A.SUB_CAP, A.SUB_CAP), (ONE - 1, ONE - 1), (A.SUB_CAP, MUL1), (MUL1, A.SUB_CAP),
                   (2 * MUL1, ADD3), (3 * ONE + 0x12ff, 0)):
        pa, pb = patterns(ca, rng, 24), patterns(cb, rng, 24)
        n = len(pa)
        sub += [(pa[i], pb[(i + s) % len(pb)]) for s in (0, 3) for i in range(n)]
        sub += [(a, list(a)) for a in pa]  # b limb-wise equal to a
    # the carry into limb 0 is (limb 8 >> 29) * 1216: limb 8 of a + 4 Z1 - b at 7 * 2^29
    sub.append(([3 * ONE + 0x12ff, 0, 0, 0, 0, 0, 0, 0, 3 * ONE + 4], [0] * 9))
    for a, b in sub:
        assert max(a) <= A.SUB_CAP and max(b) <= A.SUB_CAP
    c["kOpFeSub"] = _arr([_row(p) for p in sub])

    neg = patterns(A.Z1_4, rng, 60)
    c["kOpFeNeg"] = _arr([_row([a]) for a in neg])
    for name, k in (("kOpFeSubNc2", 2), ("kOpFeSubNc3", 3)):
        pb = patterns([k * z for z in A.Z1], rng, 40)
        pa = patterns((1 << 32) - 1 - k * M29, rng, 40)
        n = len(pa)
        rows = [(pa[i], pb[(i + s) % len(pb)]) for s in (0, 1, 4) for i in range(n)]
        for a, b in rows:
            assert all(b[i] <= k * A.Z1[i] for i in range(9)) and max(a) + k * M29 < 1 << 32
        c[name] = _arr([_row(p) for p in rows])
    c["kOpFeNegNc2"] = _arr([_row([a]) for a in patterns([2 * z for z in A.Z1], rng, 40)])
    c["kOpFeCarry"] = _arr([_row([a]) for cap in ((1 << 32) - 1, 7 * ONE, 7 * ONE - 1, ONE)
                            for a in patterns(cap, rng, 40)])
    wide = patterns((1 << 32) - 1, rng, 30)
    c["kOpFeCmov"] = _arr([_row([a, b], at={18: f}) for f in (0, 1, 2, 0xFFFFFFFF)
                           for a, b in zip(wide, wide[5:] + wide[:5])])

    enc = []
    for x in SPECIAL + [rng.getrandbits(256) for _ in range(64)] + [(1 << 256) - 1, 1 << 255, (1 << 232) - 1, 1 << 232]:
        x &= (1 << 256) - 1
        enc += [x, x ^ (1 << 255)]  # bit 255 both clear and set
    c["kOpFeFrombytes"] = _arr([_row(words=A.words(x, 8)) for x in enc])

    full = full_reduce_inputs(rng)
    for name in ("kOpFeTobytes", "kOpFeIszero", "kOpFeIsnegative"):
        c[name] = _arr([_row([a]) for a in full])

    inv = [A.to_limbs(x) for x in (0, 1, P - 1, ed.SQRTM1, P - ed.SQRTM1, 2, P - 2)]
    inv += patterns(MUL1, rng, 256 - len(inv) - 29)[:256 - len(inv)]
    assert len(inv) == 256 and all(max(a) <= MUL1 for a in inv)
    c["kOpFeInvert"] = _arr([_row([a]) for a in inv])
    c["kOpFePow22523"] = c["kOpFeInvert"]
    for name in ("kOpFeConstD", "kOpFeConst2d", "kOpFeConstSqrtm1"):
        c[name] = _arr([_row(), _row([[0xFFFFFFFF] * 9] * 8)])  # the input row is ignored
    return c


def full_reduce_inputs(rng):
    """fe_tobytes / fe_iszero / fe_isnegative: any representative below 2^262
    (limbs at most 2^32 - 8: the first carry pass adds up to 7 to a limb)."""
    top = (1 << 30) - 16
    out = []
    for cap in (ONE - 1, MUL1, A.CARRY_OUT, 2 * ONE - 1, 3 * ONE, 7 * ONE, (1 << 32) - 8):
        out += patterns([cap] * 8 + [min(cap, top)], rng, 24)
    for k in (0, 1, 2, 3, 64, 127, 128):
        for x in (k * P - 1, k * P, k * P + 1):
            if x < 0:
                continue
            base = A.to_limbs(x)
            out.append(base)
            for i in range(8):  # the same value, not normalised: 2^29 moved from limb i+1 into limb i
                if base[i + 1] >= 1:
                    v = list(base)
                    v[i] += ONE
                    v[i + 1] -= 1
                    assert A.value(v) == x
                    out.append(v)
    for a in out:
        assert A.value(a) < 1 << 262 and max(a) <= (1 << 32) - 8
    return out


# ---- scalars ------------------------------------------------------------

def reduce64_inputs():
    """q*L + {0, 1, L-2, L-1} for q around every power of two and at the top
    of the range, and 2^b, 2^b - 1, 2^512 - 2^b for every b."""
    top = 1 << 512
    qmax = (top - 1) // L
    qs = {max(0, min(qmax, (1 << j) + d)) for j in range(qmax.bit_length() + 1) for d in (-2, -1, 0, 1, 2)}
    qs |= {qmax - d for d in range(5)} | {0, 1, 2}
    xs = []
    for q in sorted(qs):
        xs += [q * L + r for r in (0, 1, L - 2, L - 1) if q * L + r < top]
    for b in range(513):
        xs += [x for x in ((1 << b), (1 << b) - 1, top - (1 << b)) if 0 <= x < top]
    xs.append(top - 1)
    assert len(xs) >= 4096
    return xs


def recode_scalars(rng):
    f = lambda pat: int(pat * (64 // len(pat)), 16) & ((1 << 253) - 1)  # noqa: E731
    xs = [0, 1, L - 1, L, (1 << 253) - 1, f("8"), f("7"), (1 << 252) - 1, 1 << 252, f("7f"), f("80"), f("7fff"),
          f("8000"), f("0f"), f("f0")]
    xs += [rng.getrandbits(253) for _ in range(300)] + [rng.randrange(L) for _ in range(100)]
    assert all(0 <= x < 1 << 253 for x in xs)
    return xs


def lattice_ks(rng):
    """Boundary and Fibonacci k spread so that every 64-row wave holds at
    least one of them next to random ones; 4,000 random k in all."""
    hard = _boundary_ks() + _fib_ks()
    rand = [rng.randrange(L) for _ in range(4000)]
    waves = -(-(len(hard) + len(rand)) // 64)
    ks, hi, ri = [], 0, 0
    for w in range(waves):
        take = len(hard) * (w + 1) // waves - len(hard) * w // waves
        if take == 0:  # more waves than hard values: reuse them in turn
            wave = [hard[w % len(hard)]]
        else:
            wave = hard[hi:hi + take]
            hi += take
        pos = rng.randrange(64 - len(wave) + 1)
        fill = rand[ri:ri + 64 - len(wave)]
        ri += len(fill)
        ks += fill[:pos] + wave + fill[pos:]
    assert hi == len(hard)
    ks += rand[ri:]
    special = set(hard)
    assert all(any(k in special for k in ks[i:i + 64]) for i in range(0, len(ks) - 63, 64))
    return ks


def scalar_cases(rng):
    c = {}
    c["kOpScReduce64"] = _arr([_row(words=A.words(x, 16)) for x in reduce64_inputs()])
    pool = lambda: [0, 1, L - 1, L, 1 << 252, (1 << 256) - 1, rng.getrandbits(256)]  # noqa: E731
    mul = [(a, b, cc) for a in pool() for b in pool() for cc in pool()]
    mul += [(rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(256)) for _ in range(200)]
    c["kOpScMuladd"] = _arr([_row(words=A.words(a, 8) + A.words(b, 8) + A.words(cc, 8)) for a, b, cc in mul])
    lw = A.words(L, 8)
    lt = [L, L - 1, L + 1, L + (1 << 252), 0, (1 << 256) - 1, L - (1 << 32), L + (1 << 32), (1 << 252) - 1, 1 << 252]
    lt_words = [A.words(x, 8) for x in lt]
    for i in range(8):  # L with each word changed by 1 in place (no borrow or carry)
        for d in (-1, 1):
            w = list(lw)
            w[i] = (w[i] + d) & 0xFFFFFFFF
            lt_words.append(w)
    lt_words += [A.words(rng.getrandbits(256), 8) for _ in range(64)]
    lt_words += [A.words(L - 1 - rng.getrandbits(b), 8) for b in range(1, 252, 8)]
    lt_words += [A.words(L + rng.getrandbits(b), 8) for b in range(1, 252, 8)]
    c["kOpScLtL"] = _arr([_row(words=w) for w in lt_words])
    rec = recode_scalars(rng)
    for name in ("kOpScRecode16", "kOpScRecode256", "kOpScRecode65536"):
        c[name] = _arr([_row(words=A.words(x, 8)) for x in rec])
    ms = []
    for _ in range(400):
        d = rng.choice([rng.getrandbits(158), rng.getrandbits(160), rng.getrandbits(128), 0, 1, (1 << 160) - 1])
        S = rng.choice([rng.getrandbits(256), rng.randrange(L), 0, L - 1, L, (1 << 256) - 1])
        ms.append(_row(words=A.words(d, 5) + [rng.randrange(2)], at=dict(zip(range(8, 16), A.words(S, 8)))))
    c["kOpScMulSigned"] = _arr(ms)
    c["kOpLatticeHalf"] = _arr([_row(words=A.words(k, 8)) for k in lattice_ks(rng)])
    half = [0, 1, 7, 8, 9, (1 << 158) - 1, 1 << 157, int("8" * 39, 16), int("7" * 39, 16), int("f" * 32, 16)]
    half += [rng.getrandbits(rng.randrange(1, 159)) for _ in range(300)]
    assert all(x < 1 << 158 for x in half)
    c["kOpScRecode16Half"] = _arr([_row(words=A.words(x, 5)) for x in half])
    return c


# ---- group --------------------------------------------------------------

def points(rng):
    """identity, B, the order-2, order-4 and order-8 points, B + T8 and 64
    random multiples of B (every third with a torsion point added)."""
    tors, T8 = ed.torsion_points()
    pts = [ed.IDENT, ed.B, tors[4], tors[2], T8, ed.add(ed.B, T8)]
    for i in range(64):
        p = ed.mul(rng.randrange(1, L), ed.B)
        pts.append(ed.add(p, tors[rng.randrange(8)]) if i % 3 == 0 else p)
    return pts


def repr_fe(v, k, rng, jitter=True):
    """Limbs of value == v (mod p): a product's output shape -- 29-bit limbs
    plus up to 2^17 per limb -- pushed up by k * Z1 as the lazy forms do."""
    e = [rng.randrange((1 << 17) + 1) if jitter else 0 for _ in range(9)]
    base = A.to_limbs((v - A.value(e)) % P)
    out = [base[i] + e[i] + k * A.Z1[i] for i in range(9)]
    assert (A.value(out) - v) % P == 0 and max(out) <= A.MUL_OUT + k * M29
    return out


def neg2_fe(v, rng):
    """2 Z1 - t with t a product-shaped value of -v: what fe_neg_nc<2> leaves"""
    t = repr_fe(-v, 0, rng)
    out = [2 * z - a for z, a in zip(A.Z1, t)]
    assert (A.value(out) - v) % P == 0
    return out


def _proj(pt, rng):
    z = rng.randrange(1, P)
    x, y = ed.affine(pt)
    return x * z % P, y * z % P, z, x * y * z % P


def _mul_ok(a, b):
    assert max(a) * max(b) <= A.MUL_CAP


def group_cases(rng):
    pts = points(rng)
    c = {}
    variants = (0, 1, 2)  # canonical limbs; product-shaped; pushed to the annotated input bounds
    dbl, dbl_aff, addc, madd, p1p1, p1p1_lazy, tocached, cneg, nneg, tob = [], [], [], [], [], [], [], [], [], []
    for i, pt in enumerate(pts):
        q = pts[(5 * i + 3) % len(pts)]
        for var in variants:
            jit = var > 0
            X, Y, Z, T = _proj(pt, rng)
            x, y = ed.affine(pt)
            p2 = [repr_fe(X, 0, rng, jit), repr_fe(Y, 0, rng, jit), repr_fe(Z, 0, rng, jit)]
            dbl.append(_row(p2))  # p2 [1]
            tob.append(_row(p2))
            dbl_aff.append(_row([repr_fe(x, 0, rng, jit), repr_fe(y, 0, rng, jit), A.to_limbs(1),
                                 repr_fe(x * y, 0, rng, jit)]))
            p3 = p2 + [repr_fe(T, 0, rng, jit)]
            X2, Y2, Z2, T2 = _proj(q, rng)
            t2d = 2 * ed.D * T2 % P
            cached = [repr_fe(Y2 + X2, 0, rng, jit), repr_fe(Y2 - X2, 0, rng, jit), repr_fe(Z2, 0, rng, jit),
                      neg2_fe(t2d, rng) if var == 2 else repr_fe(t2d, 0, rng, jit)]  # T2d <= 2
            addc.append(_row(p3 + cached))
            qx, qy = ed.affine(q)
            xy2d = 2 * ed.D * qx * qy % P
            niels = [repr_fe(qy + qx, 0, rng, jit), repr_fe(qy - qx, 0, rng, jit),
                     neg2_fe(xy2d, rng) if var == 2 else repr_fe(xy2d, 0, rng, jit)]
            madd.append(_row(p3 + niels))
            for neg in (0, 1):
                cneg.append(_row(cached, at={36: neg}))
                nneg.append(_row(niels, at={27: neg}))
            # p3 -> cached: [1], and pushed to X, Y [2] (fe_add [4], fe_sub <= 3.9), T [2]
            k = 1 if var == 2 else 0
            tocached.append(_row([repr_fe(X, k, rng, jit), repr_fe(Y, k, rng, jit), repr_fe(Z, 0, rng, jit),
                                  repr_fe(T, k, rng, jit)]))
            # p1p1 ((X:Z),(Y:T)): X [3], Y [2], Z [3], T [1] as dbl / add / madd leave them
            zz, tt = rng.randrange(1, P), rng.randrange(1, P)
            kx, ky, kz = (2, 1, 2) if var == 2 else (0, 0, 0)
            pp = [repr_fe(x * zz, kx, rng, jit), repr_fe(y * tt, ky, rng, jit), repr_fe(zz, kz, rng, jit),
                  repr_fe(tt, 0, rng, jit)]
            p1p1.append(_row(pp))
            p1p1_lazy.append(_row([repr_fe(x * zz, 3 if var == 2 else 0, rng, jit)] + pp[1:]))  # lazy X [4]
    for r in p1p1:
        X, Y, Z, T = (r[9 * j:9 * j + 9] for j in range(4))
        for a, b in ((X, T), (Y, Z), (Z, T), (X, Y)):
            _mul_ok(a, b)
    for r in p1p1_lazy:
        X, Y, Z, T = (r[9 * j:9 * j + 9] for j in range(4))
        for a, b in ((X, T), (Y, Z), (Z, T)):
            _mul_ok(a, b)
    for r in tocached:
        assert max(r[:18]) <= A.SUB_CAP
    for rows, t2d_slot in ((addc, 7), (madd, 6), (cneg, 3), (nneg, 2)):
        for r in rows:
            t = r[9 * t2d_slot:9 * t2d_slot + 9]
            assert all(t[i] <= 2 * A.Z1[i] for i in range(9))  # fe_neg_nc<2>'s limb-wise condition
    c["kOpGeP2Dbl"] = _arr(dbl)
    c["kOpGeP2DblLazy"] = c["kOpGeP2Dbl"]
    c["kOpGeAffineDbl"] = _arr(dbl_aff)
    c["kOpGeAddCached"] = _arr(addc)
    c["kOpGeMadd"] = _arr(madd)
    c["kOpGeP1p1ToP2"] = _arr(p1p1 + p1p1_lazy)
    c["kOpGeP1p1ToP3"] = _arr(p1p1)
    c["kOpGeP3ToCached"] = _arr(tocached)
    c["kOpGeCachedCneg"] = _arr(cneg)
    c["kOpGeNielsCneg"] = _arr(nneg)
    c["kOpGeTobytes"] = _arr(tob)

    enc = [ed.encode(p) for p in pts]
    enc += [bytes(b) for b in ed.SMALL_ORDER_BLOCKLIST]
    enc += [(y | (s << 255)).to_bytes(32, "little") for y in (0, 1, 2, P - 1, P, P + 1, (1 << 255) - 1) for s in (0, 1)]
    enc += [rng.getrandbits(256).to_bytes(32, "little") for _ in range(64)]  # about half are off the curve
    enc += [bytes([e[0]]) + e[1:31] + bytes([e[31] ^ 0x80]) for e in enc[:70]]
    c["kOpGeFrombytesNegate"] = _arr([_row(words=A.words(int.from_bytes(e, "little"), 8)) for e in enc])
    return c


# the one-lane op whose rows (and host results) each lane-group op restates
GROUP_MAP = {"kGrpMul4": "kOpFeMul4", "kGrpSq4": "kOpFeSq4", "kGrpP2Dbl": "kOpGeP2Dbl", "kGrpToP3": "kOpGeP1p1ToP3",
             "kGrpToP2": "kOpGeP1p1ToP3", "kGrpAddCached": "kOpGeAddCached", "kGrpMadd": "kOpGeMadd"}


@functools.lru_cache(maxsize=None)
def cases():
    rng = random.Random(0x51E1F7E5)
    c = {}
    c.update(field_cases(rng))
    c.update(scalar_cases(rng))
    c.update(group_cases(rng))
    assert set(c) == set(A.OPS), set(A.OPS) ^ set(c)
    for a in c.values():
        a.setflags(write=False)
    return c
