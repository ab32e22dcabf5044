"""CPU-only checks of the fixed-base multiplication's digit recoding: the pure-Python model
(tests/fixed_base_model.py) and the library's own host recoding (mbls_fixed_base_recode, the function
the kernels run) go through the same cases, for the digit width the plan reports, and must give the
same digits.

The property the kernels lean on: for a base of order r the accumulation never adds a point to
itself or to its negative -- no partial sum is +- the next addend mod r -- so madd's doubling and
cancellation branches are reached only through its identity branch at the first non-zero digit."""
import os
import random
import subprocess
import sys

import pytest

import fixed_base_model as M
import helpers as H

PKG = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd")
LIB = os.path.join(PKG, "lib", "libbls12_381_mi355x.so")


@pytest.fixture(scope="module")
def amd():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", PKG, "-j8", "-s"])
    sys.path.insert(0, PKG)
    import bls12_381_amd
    bls12_381_amd.lib()
    return bls12_381_amd


@pytest.fixture(scope="module")
def cases(amd):
    c = amd.fixed_base_plan("g1")["c"]
    rnd = random.Random(0xF1BA5E01)
    return c, M.edge_scalars(c) + [rnd.randrange(M.R) for _ in range(10000)]


def test_plan_width_is_one_for_both_groups(amd):
    p1, p2 = amd.fixed_base_plan("g1"), amd.fixed_base_plan("g2")
    assert (p1["c"], p1["W"], p1["rows"]) == (p2["c"], p2["W"], p2["rows"])
    assert p1["W"] == M.windows(p1["c"])


def test_digits_sum_to_the_scalar_and_stay_in_bounds(cases):
    c, sc = cases
    W, half = M.windows(c), 1 << (c - 1)
    top_max = 0
    for k in sc:
        d = M.recode(k, c)
        assert len(d) == W
        assert sum(v << (c * w) for w, v in enumerate(d)) == k % M.R, hex(k)
        assert all(-half <= v <= half - 1 for v in d[:-1]), hex(k)
        assert 0 <= d[-1] <= half, hex(k)
        assert all(0 <= M.table_index(w, v, c) < W * half for w, v in enumerate(d) if v), hex(k)
        assert all(M.table_scalar(M.table_index(w, v, c), c) == abs(v) << (c * w) for w, v in enumerate(d) if v)
        top_max = max(top_max, d[-1])
    # the top digit does not decrease with k, so the largest is that of r - 1 (in the edge list): the
    # top window of r - 1, plus a carry where the window below it reaches 2^(c-1) (it does at c = 8
    # and 10, not at 12)
    assert top_max == M.recode(M.R - 1, c)[-1] <= ((M.R - 1) >> (c * (W - 1))) + 1 <= half
    assert [M.recode(M.R - 1, w)[-1] for w in (8, 10, 12)] == [0x74, 0x1d, 7]


def test_no_partial_sum_is_plus_or_minus_the_next_addend(cases):
    c, sc = cases
    for k in sc:
        assert not M.meets_exception(M.recode(k, c), c), hex(k)


def test_the_property_is_not_vacuous():
    """a digit string that does double is seen by the model: 1 + 1 at two rows of the same window
    cannot come out of recode, so it is written by hand"""
    assert M.partial_sums([3, 0, 1], 8) == [(0, 3), (3, 1 << 16)]
    assert M.meets_exception([1, 0], 8) is False
    # partial sum 2^8, next addend 2^8 expressed as digit 1 of window 1 after a hand-made first window
    assert M.meets_exception([1 << 8, 1], 8) is True
    assert M.meets_exception([-(1 << 8), 1], 8) is True


def test_library_recoding_gives_the_model_digits(amd, cases):
    c, sc = cases
    for k in sc:
        assert amd.fixed_base_recode(k) == M.recode(k, c), hex(k)
    # any 256-bit value is reduced first
    for k in (M.R, M.R + 5, 2 * M.R + 1, (1 << 256) - 1):
        assert amd.fixed_base_recode(k) == M.recode(k % M.R, c), hex(k)
