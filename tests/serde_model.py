"""The compressed point encoding (mbls_g*_compress / mbls_g*_decompress) in pure Python on
oracle/pyref.py integers, by the format's definition alone, and the records the tests feed the GPU.

G1: 48 bytes, x big-endian.  G2: 96 bytes, x.c1 then x.c0.  The top three bits of byte 0: C (bit 7)
always set, I (bit 6) infinity with every other bit zero, S (bit 5) y is the larger of {y, -y} --
y > (p - 1) / 2, for G2 on y.c1, and on y.c0 only when y.c1 == 0.

decode's tests run in the order BAD_FLAGS, IDENTITY, NONCANONICAL, NO_POINT and the first failure
is the status; a point is returned for OK only (None otherwise: the kernel writes the all-zero
point).  Roots come from subgroup_cases.fp_sqrt / fp2_sqrt."""
import functools
import random

import numpy as np

import subgroup_cases as S
from helpers import pyref as pr

P = pr.P
OK, IDENTITY, NONCANONICAL, NO_POINT, BAD_FLAGS = 0, 1, 2, 3, 5
C_BIT, I_BIT, S_BIT = 0x80, 0x40, 0x20
SIZE = {"g1": 48, "g2": 96}
HALF = (P - 1) // 2

G1_HEX = "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
G2_HEX = ("93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
          "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")


# ---------------------------------------------------------------------------- the format
def y_is_larger(group, y):
    if group == "g1":
        return y > HALF
    return y[1] > HALF or (y[1] == 0 and y[0] > HALF)


def infinity(group):
    return bytes([C_BIT | I_BIT]) + bytes(SIZE[group] - 1)


def raw_record(group, x, flags):
    """the record of the integer x (G2: (c0, c1)), each < 2^381 for the flags to stay apart, with
    the given flag bits, whatever they say"""
    body = x.to_bytes(48, "big") if group == "g1" else x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big")
    return bytes([body[0] | flags]) + body[1:]


def encode(group, pt):
    if pt is None:
        return infinity(group)
    x, y = pt
    return raw_record(group, x, C_BIT | (S_BIT if y_is_larger(group, y) else 0))


def decode(group, data):
    """(status, point): the point for OK, else None"""
    assert len(data) == SIZE[group]
    flags = data[0] & 0xE0
    body = bytes([data[0] & 0x1F]) + data[1:]
    if not flags & C_BIT:
        return BAD_FLAGS, None
    if flags & I_BIT:
        return (BAD_FLAGS if flags & S_BIT or any(body) else IDENTITY), None
    if group == "g1":
        x = int.from_bytes(body, "big")
        if x >= P:
            return NONCANONICAL, None
        y = S.fp_sqrt(x * x * x + pr.G1_B)
        neg = None if y is None else (P - y) % P
    else:
        x = (int.from_bytes(body[48:], "big"), int.from_bytes(body[:48], "big"))
        if x[0] >= P or x[1] >= P:
            return NONCANONICAL, None
        y = S.fp2_sqrt(pr.f2_add(pr.f2_mul(pr.f2_mul(x, x), x), pr.G2_B))
        neg = None if y is None else pr.f2_neg(y)
    if y is None:
        return NO_POINT, None
    if y_is_larger(group, y) != bool(flags & S_BIT):
        y = neg
    return OK, (x, y)


def to_array(group, records):
    """(n, 48 | 96) uint8"""
    return np.frombuffer(b"".join(records), dtype=np.uint8).reshape(len(records), SIZE[group]).copy()


def words(group, pts, mont=True):
    """the affine words of points (None: the all-zero point), (n, 12 | 24) uint64"""
    return S.encode(group, [S.case(group, p) for p in pts], mont=mont)


def decoded(group, records):
    """(statuses as uint8, points with None for every status but OK) of a list of records"""
    out = [decode(group, r) for r in records]
    return np.array([s for s, _ in out], dtype=np.uint8), [p for _, p in out]


# ---------------------------------------------------------------------------- case builders
def radicand(group, x):
    if group == "g1":
        return (x * x * x + pr.G1_B) % P
    return pr.f2_add(pr.f2_mul(pr.f2_mul(x, x), x), pr.G2_B)


@functools.lru_cache(maxsize=None)
def no_point_xs(group, k=3):
    """the first k x of a seeded stream for which x^3 + b is not a square"""
    rnd = random.Random(0x5E4D01 if group == "g1" else 0x5E4D02)
    out = []
    while len(out) < k:
        x = rnd.randrange(P) if group == "g1" else (rnd.randrange(P), rnd.randrange(P))
        root = S.fp_sqrt(radicand(group, x)) if group == "g1" else S.fp2_sqrt(radicand(group, x))
        if root is None:
            out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def malformed(group):
    """(record, status) of every malformed kind the format has"""
    gen = S.ops(group)[3]
    n = SIZE[group]
    good = encode(group, gen)
    inf = infinity(group)
    lift = (lambda v: v) if group == "g1" else (lambda v: (gen[0][0], v))   # G2: x.c1 carries the value
    out = [(bytes([good[0] & 0x7F]) + good[1:], BAD_FLAGS),                   # C clear
           (bytes(n), BAD_FLAGS),                                            # all zero: C clear
           (bytes([inf[0] | S_BIT]) + inf[1:], BAD_FLAGS),                   # I with S
           (inf[:-1] + b"\x01", BAD_FLAGS),                                  # I with one low bit
           (bytes([inf[0] | 0x10]) + inf[1:], BAD_FLAGS),                    # I with the top bit of x
           (bytes([inf[0] & 0x7F]) + inf[1:], BAD_FLAGS)]                    # I without C
    if group == "g2":
        out.append((inf[:48] + b"\x80" + inf[49:], BAD_FLAGS))               # I with a bit in the second half
        out.append((inf[:95] + b"\x01", BAD_FLAGS))
    for v in (P, P + 1, (1 << 381) - 1):
        for s in (0, S_BIT):
            out.append((raw_record(group, lift(v), C_BIT | s), NONCANONICAL))
    if group == "g2":
        for v in (P, (1 << 381) - 1, (1 << 384) - 1):                        # only x.c0 >= p
            out.append((raw_record(group, (v, gen[0][1]), C_BIT), NONCANONICAL))
        out.append((raw_record(group, (P, P), C_BIT), NONCANONICAL))
    for x in no_point_xs(group):
        out.append((raw_record(group, x, C_BIT), NO_POINT))
        out.append((raw_record(group, x, C_BIT | S_BIT), NO_POINT))
    return tuple(out)


def _cube_root(c):
    """a cube root of c in Fp or None.  p - 1 = 3^s t with 3 not dividing t: r = c^(1 / 3 mod t) has
    r^3 = c w for a w of the order-3^s subgroup, which is small enough to walk"""
    c %= P
    s, t = 0, P - 1
    while t % 3 == 0:
        s, t = s + 1, t // 3
    h = 2
    while pow(pow(h, t, P), 3 ** (s - 1), P) == 1:
        h += 1
    z = pow(h, t, P)                              # a generator of the order-3^s subgroup
    r = pow(c, pow(3, -1, t), P)
    for _ in range(3 ** s):
        if pow(r, 3, P) == c:
            return r
        r = r * z % P
    return None


@functools.lru_cache(maxsize=None)
def g1_specials():
    """curve points (not subgroup members) on the edges of the S rule: x = 0 with y = +-2, and the
    points whose y lie closest to (p - 1) / 2 on either side, so that the comparison is decided in
    the lowest word"""
    pts = [(0, 2), (0, P - 2)]
    for step in (1, -1):
        y = HALF + (1 if step > 0 else 0)        # the smallest "larger" y, the largest "smaller" y
        while True:
            x = _cube_root(y * y - pr.G1_B)
            if x is not None:
                break
            y += step
        pts += [(x, y), (x, P - y)]
    return tuple(pts)


@functools.lru_cache(maxsize=None)
def g2_specials():
    """curve points (not subgroup members) that walk the Fq2 root's branches.  With x0^2 =
    (x1^3 - 4) / (3 x1) the radicand c = x^3 + b is real: one x with c a square (y = (s, 0), S
    decided on c0), one with c a non-square (y = (0, t)).  And x = (k, 0) for k = 2, 4, 5."""
    rnd = random.Random(0x5E4D03)
    found = {}
    while len(found) < 2:
        x1 = rnd.randrange(1, P)
        x0 = S.fp_sqrt((pow(x1, 3, P) - 4) * pow(3 * x1, -1, P))
        if x0 is None:
            continue
        c = radicand("g2", (x0, x1))
        assert c[1] == 0 and c[0] != 0
        y = S.fp2_sqrt(c)
        kind = "real" if y[1] == 0 else "imaginary"
        assert (y[0] == 0) != (y[1] == 0)
        found.setdefault(kind, ((x0, x1), y))
    pts = [found["real"], found["imaginary"]]
    for k in (2, 4, 5):
        pt = S.curve_point("g2", None, x=(k, 0))
        assert pt is not None, k
        pts.append(pt)
    return tuple(pts + [(x, pr.f2_neg(y)) for x, y in pts])


@functools.lru_cache(maxsize=None)
def member_points(group, n=12):
    """the generator, [r - 1] G (the opposite sign of y) and n members"""
    gen = S.ops(group)[3]
    mul = pr.g1_mul if group == "g1" else pr.g2_mul
    return (gen, mul(pr.R - 1, gen)) + tuple(mul(0xC0FFEE + 977 * k, gen) for k in range(n))


@functools.lru_cache(maxsize=None)
def status_table(group):
    """(records, statuses, points) of the status and value table: the valid points of every kind,
    infinity and every malformed kind"""
    special = g1_specials() if group == "g1" else g2_specials()
    records = [encode(group, p) for p in member_points(group) + special] + [infinity(group)]
    records += [r for r, _ in malformed(group)]
    st, pts = decoded(group, records)
    return tuple(records), st, tuple(pts)
