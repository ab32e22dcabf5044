"""CPU-only: the tiled scan scheme of csrc/scan.hip, as modelled in tests/scan_model.py at toy
geometry, equals the sequential recurrences at every seam size; the division identity holds
coefficient by coefficient; and the two readings of a zero denominator agree."""
import random

import pytest

import scan_model as M
from helpers import pyref as pr

# K = 4 elements per thread, 2 waves of 4 lanes: tiles of 32; up to 16 workgroups
G1 = M.Geometry(K=4, wave=4, waves=2, tpg=1, agg_k=2)
G2 = G1._replace(tpg=2)  # spans of two tiles


def _sizes(g):
    t, span = M.tile_elems(g), g.tpg * M.tile_elems(g)
    return sorted({1, 2, g.K - 1, g.K, g.K + 1, t - 1, t, t + 1, span - 1, span, span + 1, 2 * span + 3})


def _column(n, seed):
    """Montgomery values mixing 0, 1, r - 1 and random ones"""
    rnd = random.Random(seed)
    return [M.mont(rnd.choice([0, 1, M.R - 1] + [rnd.randrange(M.R)] * 9)) for _ in range(n)]


def _points(seed):
    return [M.mont(v) for v in (0, 1, M.R - 1, random.Random(seed).randrange(M.R))]


@pytest.mark.parametrize("g", [G1, G2], ids=["one_tile_spans", "two_tile_spans"])
def test_tiled_horner_equals_the_recurrence(g):
    for n in _sizes(g):
        a = _column(n, n)
        for z in _points(n):
            assert M.tiled_scan(M.HORNER, a, g, unit=z) == M.divide_ref(a, z), (n, z)


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("g", [G1, G2], ids=["one_tile_spans", "two_tile_spans"])
def test_tiled_product_equals_the_recurrence(g, inclusive):
    for n in _sizes(g):
        x = _column(n, 100 + n)
        nz = [v or M.ONE for v in x]  # and a column without zeros, whose tail stays alive
        init = M.mont(random.Random(n).randrange(1, M.R))
        for col in (x, nz):
            want = M.prefix_product_ref(col, None, init, inclusive)
            assert M.tiled_scan(M.MUL, col, g, init=init, inclusive=inclusive) == want, n
    # the default carry-in is Montgomery one
    assert M.tiled_scan(M.MUL, nz, g) == M.prefix_product_ref(nz)


def test_reference_product_is_the_plain_product():
    vals = [3, 5, 7, 11]
    out, total = M.prefix_product_ref([M.mont(v) for v in vals], init=M.mont(2))
    assert [pr.fr_from_mont(v) for v in out] == [2, 6, 30, 210] and pr.fr_from_mont(total) == 2310
    out, total = M.prefix_product_ref([M.mont(v) for v in vals], [M.mont(3), M.mont(1), M.mont(0), M.mont(1)],
                                      inclusive=True)
    assert [pr.fr_from_mont(v) for v in out] == [1, 5, 0, 0] and total == 0


@pytest.mark.parametrize("n", [1, 2, 33, 100])
def test_division_identity_coefficient_by_coefficient(n):
    a = _column(n, 7 * n)
    for z in _points(n):
        q, ev = M.divide_ref(a, z)
        assert q[n - 1] == 0
        # p = q * (X - z) + p(z): a[0] = p(z) - z q[0], a[i] = q[i-1] - z q[i]
        A, Q, Z = ([pr.fr_from_mont(v) for v in a], [pr.fr_from_mont(v) for v in q], pr.fr_from_mont(z))
        assert A[0] == (pr.fr_from_mont(ev) - Z * Q[0]) % M.R
        for i in range(1, n):
            assert A[i] == (Q[i - 1] - Z * Q[i]) % M.R, i
        assert pr.fr_from_mont(ev) == sum(c * pow(Z, i, M.R) for i, c in enumerate(A)) % M.R


def test_zero_denominators_both_readings_agree():
    """prefix(num) * inv(prefix(den)) and the scan of num * inv(den) agree when 1 / 0 = 0: a zero in
    either column kills every later product"""
    rnd = random.Random(5)
    for trial in range(20):
        n = rnd.randrange(1, 40)
        num, den = _column(n, 2 * trial), _column(n, 2 * trial + 1)
        for inclusive in (False, True):
            pn, tn = M.prefix_product_ref(num, inclusive=inclusive)
            pd, td = M.prefix_product_ref(den, inclusive=inclusive)
            out, total = M.prefix_product_ref(num, den, inclusive=inclusive)
            assert out == [M.mmul(x, M.minv(y)) for x, y in zip(pn, pd)]
            assert total == M.mmul(tn, M.minv(td))
            ratio = [M.mmul(x, M.minv(y)) for x, y in zip(num, den)]
            assert (out, total) == M.prefix_product_ref(ratio, inclusive=inclusive)
            first = min([i for i in range(n) if num[i] == 0 or den[i] == 0], default=n)
            tail = out[first + (0 if inclusive else 1):]
            assert all(v == 0 for v in tail) and all(v != 0 for v in out[:len(out) - len(tail)])
