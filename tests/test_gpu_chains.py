"""The packed mad chains of the radix-2^28 Fq products, limb for limb against Python integers.

csrc/mbls_madchain.hpp emits a product column in as few asm statements as its terms allow, and the
step that closes column k opens column k + 1's statement.  r28::mul, sqr, mul2 and mul4 are its four
users.  A wrong operand order, a dropped term or a misplaced shift changes the value, so every case
is compared exactly: for products sum a_i b_i the Montgomery multiplier m = -sum p^-1 mod 2^392 is
unique (its radix-2^28 digits are the m_k of the columns), hence so is (sum + m p) / 2^392 and its 14
output limbs (13 normalised, the top one holding the rest).

Inputs: 0, 1, p - 1, R' mod p; every limb at the maximum the header of mbls_fq28.hpp allows for that
operand (normalised 2^28 - 1, the minuend-plus-bias forms of sub<B16> / <B32> / <B512>, x4(x2(.)) at
2^31); 256 random values.  Each case is first checked against the header's column bound, so a case
that overflowed a column would fail here as the test's own mistake, not as the device's.
Runs through tests/diag/libchains_diag.so (the same headers, one product per lane)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import helpers as H
from helpers import pyref as pr

pytestmark = pytest.mark.gpu

CSRC = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd", "csrc")
DIAG = os.path.join(H.ROOT, "tests", "diag", "libchains_diag.so")
P = pr.P
NL, M28, RP = 14, (1 << 28) - 1, 1 << 392
MINV = (-pow(P, -1, RP)) % RP


def _carray(src, name):
    m = re.search(r"\b" + name + r"\[[^\]]*\]\s*=\s*\{([^}]*)\}", src)
    assert m, name
    return [int(v.strip().rstrip("uU"), 16) for v in m.group(1).split(",") if v.strip()]


FQ28 = open(os.path.join(CSRC, "mbls_fq28.hpp")).read()
B16, B32, B512, ONE28 = (_carray(FQ28, n) for n in ("B16", "B32", "B512", "ONE"))


def val(limbs):
    return sum(int(v) << (28 * i) for i, v in enumerate(limbs))


def limbs(x):
    return [(x >> (28 * i)) & M28 for i in range(NL - 1)] + [x >> (28 * (NL - 1))]


def expected(pairs):
    s = sum(val(a) * val(b) for a, b in pairs)
    r = (s + (s * MINV % RP) * P) >> 392
    out = limbs(r)
    assert out[-1] < 1 << 32
    return out


def column_bound_ok(pairs, square=False):
    """the header's bound with the operands' own limb maxima: every column stays below 2^64 (a
    square's column: 7 cross terms against the doubled operand and the diagonal term)"""
    terms = sum((2 * 7 + 1 if square else NL) * max(a) * max(b) for a, b in pairs)
    return terms + NL * (1 << 56) + (1 << 36) < 1 << 64


rng = random.Random(0x28C4)
NORM_MAX = [M28] * NL                                 # every limb at 2^28 - 1
SUB16 = [M28 + b for b in B16]                        # sub<B16>(a, 0), a normalised: < 2^29.6
SUB32 = [(1 << 29) - 1 + b for b in B32]              # sub<B32>(a, 0), a limbs < 2^29: < 2^30.3
SUB512 = [M28 + b for b in B512]                      # sub<B512>(a, 0): < 2^30.5
X8 = [M28 << 3] * NL                                  # x4(x2(.)) of normalised limbs: < 2^31
SPECIAL = [limbs(0), limbs(1), limbs(P - 1), ONE28]
RANDOM = [limbs(rng.randrange(P)) for _ in range(256)]


def rnd():
    return RANDOM[rng.randrange(len(RANDOM))]


def cases_mul():
    c = [(a, b) for a in SPECIAL for b in SPECIAL]
    wide = [NORM_MAX, SUB16, SUB32, SUB512, X8]
    c += [(a, NORM_MAX) for a in wide] + [(NORM_MAX, a) for a in wide] + [(SUB16, SUB16), (SUB32, SUB16)]
    c += [(a, RANDOM[(i * 7 + 1) % 256]) for i, a in enumerate(RANDOM)]
    return [[p] for p in c]


def cases_sqr():
    c = SPECIAL + [NORM_MAX, SUB16, [(1 << 29) - 1] * NL] + RANDOM
    return [[(a, a)] for a in c]


def cases_mul2():
    c = [[(a, b), (b, a)] for a in SPECIAL for b in SPECIAL]
    # the lazy Y3: a carried R against a sub<B16> form, plus neg<B16>(y) against a normalised product
    c += [[(NORM_MAX, SUB16), (B16, NORM_MAX)], [(SUB16, NORM_MAX), (NORM_MAX, B32)], [(NORM_MAX, SUB32), (SUB16, NORM_MAX)],
          [(SUB16, SUB16), (NORM_MAX, NORM_MAX)]]
    c += [[(a, rnd()), (rnd(), rnd())] for a in RANDOM]
    # distinct operands in every slot: a swapped or repeated operand changes the sum
    return c


def cases_mul4():
    c = [[(a, b), (b, a), (a, a), (b, b)] for a in SPECIAL for b in SPECIAL]
    c += [[(SUB16, NORM_MAX)] * 4, [(NORM_MAX, SUB16), (SUB16, NORM_MAX), (B16, NORM_MAX), (NORM_MAX, NORM_MAX)]]
    c += [[(a, rnd()), (rnd(), rnd()), (rnd(), rnd()), (rnd(), rnd())] for a in RANDOM]
    return c


@pytest.fixture(scope="module")
def run():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    if not os.path.exists(DIAG):
        pytest.fail(f"{DIAG} not built (__graft_entry__.build())")
    L = ctypes.CDLL(DIAG)
    L.chains_diag_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.chains_diag_run.restype = ctypes.c_int
    iw, ow = L.chains_diag_in_words(), L.chains_diag_out_words()

    def go(op, cases):
        """cases: lists of (a, b) limb pairs; operand slots x0, x1, x2, .. in that order"""
        a = np.zeros((len(cases), iw), dtype=np.uint32)
        for i, pairs in enumerate(cases):
            ops = [v for p in pairs for v in p] if op != 1 else [pairs[0][0]]
            for k, v in enumerate(ops):
                a[i, 16 * k:16 * k + NL] = v
        o = np.zeros((len(cases), ow), dtype=np.uint32)
        rc = L.chains_diag_run(op, a.ctypes.data, o.ctypes.data, len(cases))
        assert rc == 0, rc
        return o
    return go


@pytest.mark.parametrize("op,make", [(0, cases_mul), (1, cases_sqr), (2, cases_mul2), (3, cases_mul4)],
                         ids=["mul", "sqr", "mul2", "mul4"])
def test_packed_products_are_limb_exact(run, op, make):
    cases = make()
    assert len(cases) >= 256 + 4
    for pairs in cases:
        assert column_bound_ok(pairs, square=op == 1), pairs
    got = run(op, cases)
    bad = [(i, [int(v) for v in got[i, :NL]], expected(pairs)) for i, pairs in enumerate(cases)
           if [int(v) for v in got[i, :NL]] != expected(pairs)]
    assert not bad, f"{len(bad)} of {len(cases)} cases differ; first: case {bad[0][0]} got {bad[0][1]} want {bad[0][2]}"
