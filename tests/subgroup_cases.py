"""Points for the validation tests (mbls_g*_check_points), built and judged on the CPU by the
definition alone: a point is valid when its coordinates are canonical, it satisfies the curve
equation and [r]P == O for an UNREDUCED double-and-add (oracle/pyref.py's g*_mul reduce the scalar
mod r, so they cannot tell a non-member from a member).

Also the model of the two endomorphism criteria the kernel runs (Scott, "A note on group membership
tests for G1, G2 and GT on BLS pairing-friendly curves"), with pyref's beta and psi:
    G1: phi(P) + P == [z^2] P          G2: psi(P) == [z] P = -[|z|] P

A case is (coords, addp): the standard-form coordinates (G1: x, y; G2: x.c0, x.c1, y.c0, y.c1) and
per coordinate whether p is added to its ENCODED words (a non-canonical encoding of the same
value).  `encode` gives the words in Montgomery or standard form."""
import functools
import random

import numpy as np

import helpers as H
from helpers import pyref as pr

P, R = pr.P, pr.R
Z_ABS = pr.PSI_X                      # |z| = 0xd201000000010000, z < 0
Z2 = Z_ABS * Z_ABS                    # 0xac45a4010001a4020000000100000000
OK, IDENTITY, NONCANONICAL, OFF_CURVE, OFF_SUBGROUP = range(5)

# cofactors and their prime factors with multiplicity (the last G2 factor is a 448-bit prime)
H1 = (Z_ABS + 1) ** 2 // 3            # (z - 1)^2 / 3
G1_FACTORS = ((3, 1), (11, 2), (10177, 2), (859267, 2), (52437899, 2))
_z = -Z_ABS
H2 = (_z ** 8 - 4 * _z ** 7 + 5 * _z ** 6 - 4 * _z ** 4 + 6 * _z ** 3 - 4 * _z ** 2 - 4 * _z + 13) // 9
_G2_SMALL = ((13, 2), (23, 2), (2713, 1), (11953, 1), (262069, 1))
_small = 1
for _l, _e in _G2_SMALL:
    _small *= _l ** _e
assert H2 % _small == 0
H2_BIG = H2 // _small
G2_FACTORS = _G2_SMALL + ((H2_BIG, 1),)
assert H2_BIG.bit_length() == 448
_t = 1
for _l, _e in G1_FACTORS:
    _t *= _l ** _e
assert _t == H1


def ops(group):
    """(add, neg, on_curve, generator, cofactor, factors) of a group"""
    if group == "g1":
        return pr.g1_add, pr.g1_neg, pr.g1_on_curve, pr.G1, H1, G1_FACTORS
    return pr.g2_add, pr.g2_neg, pr.g2_on_curve, pr.G2, H2, G2_FACTORS


def mul_raw(group, k, pt):
    """[k] pt for the integer k >= 0, no reduction of k"""
    add = ops(group)[0]
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, pt)
    return acc


# ---------------------------------------------------------------------------- square roots
def fp_sqrt(a):
    """a root of a in Fp (p == 3 mod 4), or None"""
    a %= P
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a else None


def fp2_sqrt(a):
    """a root of a = (a0, a1) in Fp2 = Fp[u] / (u^2 + 1) (p == 3 mod 4: through the norm, whose
    root lies in Fp), or None"""
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        s = fp_sqrt(a0)
        if s is not None:
            return (s, 0)
        return (0, fp_sqrt(-a0))  # -1 is a non-residue, so -a0 is a residue
    n = fp_sqrt(a0 * a0 + a1 * a1)
    if n is None:
        return None
    inv2 = pow(2, -1, P)
    for s in (n, -n):
        x0 = fp_sqrt((a0 + s) * inv2)
        if x0:
            x = (x0, a1 * pow(2 * x0, -1, P) % P)
            if pr.f2_eq(pr.f2_mul(x, x), (a0, a1)):
                return x
    return None


def curve_point(group, rnd, x=None):
    """a point of the curve group E(Fp) / E'(Fp2) (almost never in the order-r subgroup) with a
    random x, or the given x; None when that x has no y"""
    while True:
        if group == "g1":
            xx = rnd.randrange(P) if x is None else x
            y = fp_sqrt(xx * xx * xx + pr.G1_B)
        else:
            xx = (rnd.randrange(P), rnd.randrange(P)) if x is None else x
            y = fp2_sqrt(pr.f2_add(pr.f2_mul(pr.f2_mul(xx, xx), xx), pr.G2_B))
        if y is not None:
            return (xx, y)
        if x is not None:
            return None


# ---------------------------------------------------------------------------- the definition, the criteria
@functools.lru_cache(maxsize=None)
def in_subgroup(group, pt):
    """[r] pt == O by a plain double-and-add (pt on the curve)"""
    return mul_raw(group, R, pt) is None


def criterion(group, pt):
    """the endomorphism test the kernel runs, for a point on the curve (not the identity)"""
    add, neg = ops(group)[:2]
    if group == "g1":
        return add(pr.glv_phi(pt), pt) == mul_raw("g1", Z2, pt)
    return pr.psi(pt) == neg(mul_raw("g2", Z_ABS, pt))


# ---------------------------------------------------------------------------- non-members
@functools.lru_cache(maxsize=None)
def torsion_points(group):
    """one point of order l for every prime l of the cofactor: [r h / l^e] Q has order dividing
    l^e (the l-part need not be cyclic, so [r h / l] Q could always be O); multiply by l until the
    next multiple would be O"""
    _, _, _, _, h, factors = ops(group)
    rnd = random.Random(0x7021 if group == "g1" else 0x7022)
    out = []
    for l, e in factors:
        while True:
            t = mul_raw(group, R * h // l ** e, curve_point(group, rnd))
            if t is not None:
                break
        while True:
            nxt = mul_raw(group, l, t)
            if nxt is None:
                break
            t = nxt
        out.append(t)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def members(group, n):
    """k G for k = 1 .. n"""
    add, _, _, gen = ops(group)[:4]
    out, acc = [], None
    for _ in range(n):
        acc = add(acc, gen)
        out.append(acc)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def random_curve_points(group, n):
    rnd = random.Random(0x7031 if group == "g1" else 0x7032)
    return tuple(curve_point(group, rnd) for _ in range(n))


@functools.lru_cache(maxsize=None)
def member_plus_torsion(group):
    add, _, _, gen = ops(group)[:4]
    base = pr.g1_mul(777, gen) if group == "g1" else pr.g2_mul(777, gen)
    return tuple(add(base, t) for t in torsion_points(group))


# ---------------------------------------------------------------------------- cases
def flat(group, pt):
    """coordinates of a point (None: the identity) as a flat tuple"""
    if pt is None:
        return (0, 0) if group == "g1" else (0, 0, 0, 0)
    return tuple(pt) if group == "g1" else (pt[0][0], pt[0][1], pt[1][0], pt[1][1])


def unflat(group, c):
    return (c[0], c[1]) if group == "g1" else ((c[0], c[1]), (c[2], c[3]))


def case(group, pt, addp=None):
    c = flat(group, pt)
    return (c, tuple(addp) if addp else (False,) * len(c))


def expected(group, cs):
    """status of a case by the definition"""
    c, addp = cs
    if any(addp) or any(v >= P for v in c):
        return NONCANONICAL
    if not any(c):
        return IDENTITY
    pt = unflat(group, c)
    if not ops(group)[2](pt):
        return OFF_CURVE
    return OK if in_subgroup(group, pt) else OFF_SUBGROUP


def encode(group, cases, mont=True):
    """(n, 12 | 24) uint64 words of the cases, Montgomery or standard form"""
    rows = []
    for c, addp in cases:
        row = []
        for v, ap in zip(c, addp):
            w = (pr.fq_to_mont(v) if mont else v) + (P if ap else 0)
            assert w < 1 << 384
            row += pr.int_to_limbs(w, 6)
        rows.append(row)
    return np.array(rows, dtype=np.uint64).reshape(len(cases), 12 if group == "g1" else 24)


@functools.lru_cache(maxsize=None)
def non_members(group):
    """the distinct on-curve non-members: every torsion point, every member + torsion sum, random
    curve points, and the group's special points (G1: (0, 2) and (0, p - 2), of order 3 with
    x = 0 but not the identity; G2: a curve point with x.c1 = 0)"""
    pts = list(torsion_points(group)) + list(member_plus_torsion(group)) + list(random_curve_points(group, 8))
    if group == "g1":
        pts += [q for q in ((0, 2), (0, P - 2)) if q not in pts]  # the order-3 torsion point is one of them
    else:
        k = 1
        while curve_point("g2", None, x=(k, 0)) is None:
            k += 1
        pts.append(curve_point("g2", None, x=(k, 0)))
    return tuple(pts)


@functools.lru_cache(maxsize=None)
def status_table(group):
    """the cases of the status table, in one batch"""
    _, neg, _, gen = ops(group)[:4]
    nc = 2 if group == "g1" else 4
    m = pr.g1_mul(12345, gen) if group == "g1" else pr.g2_mul(12345, gen)
    mul = pr.g1_mul if group == "g1" else pr.g2_mul
    mc = flat(group, m)
    cases = [case(group, gen), case(group, mul(R - 1, gen)), case(group, neg(m)), case(group, None),
             case(group, m, [True] + [False] * (nc - 1)),                   # x + p in place of x
             case(group, None, [False] * (nc // 2) + [True] + [False] * (nc // 2 - 1)),  # (0, p)
             ((mc[0] ^ 1,) + mc[1:], (False,) * nc),                       # one low bit of x flipped
             (mc[nc // 2:] + mc[:nc // 2], (False,) * nc)]                  # x and y swapped
    cases += [case(group, p) for p in non_members(group)]
    return tuple(cases)
