"""CPU-only: tests/domain_model.py against pyref's NTT, against its own definitions by direct sums,
against its closed forms and against the restatement of halo2's EvaluationDomain."""
import pytest

import domain_model as D
import ntt_model as NM
from helpers import pyref as pr

R = pr.R


def _rand(seed, n):
    g = pr.rng(seed)
    return [g.randrange(R) for _ in range(n)]


SHAPES = [(1, 1), (1, 2), (2, 2), (3, 4), (3, 8), (8, 8), (5, 16), (16, 64), (17, 64), (1, 64), (64, 64)]


@pytest.mark.parametrize("size,N", SHAPES)
@pytest.mark.parametrize("gname", list(D.GENERATORS))
def test_forward_is_pad_scale_ntt(size, N, gname):
    g = D.GENERATORS[gname]
    a = _rand(size * 131 + N, size)
    want = pr.ntt_forward([(c * pow(g, i, R)) % R for i, c in enumerate(a)] + [0] * (N - size))
    assert D.coeff_to_extended(a, N, g, direct=True) == want
    assert D.coeff_to_extended(a, N, g, direct=False) == want
    if N >= 2:  # and the kernel-level model of the plain transform agrees with pr
        x = [pr.fr_to_mont(v) for v in [(c * pow(g, i, R)) % R for i, c in enumerate(a)] + [0] * (N - size)]
        assert [pr.fr_from_mont(v) for v in NM.run(x)[0]] == want


@pytest.mark.parametrize("m,N", SHAPES)
@pytest.mark.parametrize("gname", ["one", "zeta", "rand"])
@pytest.mark.parametrize("period", [None, 1, 2, "N"])
def test_inverse_is_the_composed_definition(m, N, gname, period):
    g = D.GENERATORS[gname]
    e = _rand(m * 17 + N, N)
    period = N if period == "N" else period if period is None else min(period, N)
    vinv = None if period is None else _rand(period + 5, period)
    ev = e if vinv is None else [(v * vinv[j % period]) % R for j, v in enumerate(e)]
    gi = pow(g, -1, R)
    want = [(c * pow(gi, i, R)) % R for i, c in enumerate(pr.ntt_inverse(ev))][:m]
    assert D.extended_to_coeff(e, N, m, g, vinv, direct=True) == want
    assert D.extended_to_coeff(e, N, m, g, vinv, direct=False) == want


@pytest.mark.parametrize("size,N", SHAPES + [(100, 1 << 9), (1 << 7, 1 << 10)])
def test_round_trip(size, N):
    a = _rand(size + 3 * N, size)
    for g in (1, D.ZETA, D.FIXED_RANDOM):
        assert D.extended_to_coeff(D.coeff_to_extended(a, N, g), N, size, g) == a


@pytest.mark.parametrize("j", [3, 4, 5])
def test_halo2_restatement(j):
    k = 4
    dom = D.Halo2Domain(k, j)
    assert pow(D.ZETA, 3, R) == 1 != D.ZETA
    assert dom.extended_k == {3: 5, 4: 6, 5: 6}[j]
    assert len(dom.t_evaluations) == 1 << (dom.extended_k - k)
    a = _rand(j, dom.n)
    ext = dom.coeff_to_extended(a)
    assert ext == D.coeff_to_extended(a, dom.N, D.ZETA, direct=True)
    # t_evaluations is 1 / (X^n - 1) on the coset
    for jj in (0, 1, dom.N - 1):
        x = D.ZETA * pow(dom.extended_omega, jj, R) % R
        assert dom.t_evaluations[jj % len(dom.t_evaluations)] * (pow(x, dom.n, R) - 1) % R == 1
    h = _rand(j + 9, dom.N)
    want = dom.extended_to_coeff(dom.divide_by_vanishing_poly(h))
    m = dom.n * dom.quotient_poly_degree
    assert len(want) == m
    assert D.extended_to_coeff(h, dom.N, m, D.ZETA, dom.t_evaluations, direct=True) == want
    assert D.extended_to_coeff(h, dom.N, m, D.ZETA, dom.t_evaluations, direct=False) == want


@pytest.mark.parametrize("N", [1, 2, 8, 64, 1 << 9])
def test_closed_forms(N):
    for g in (1, D.ZETA, R - 1, 7):
        for v in (1, R - 1, D.FIXED_RANDOM):
            for q in sorted({0, 1 % N, N // 2, N - 1}):
                a = [0] * q + [v]
                assert D.monomial_extended(v, q, N, g) == D.coeff_to_extended(a, N, g), (g, v, q)
            for size in sorted({1, max(1, N // 4), max(1, N // 4 - 1), N}):
                assert D.constant_run_extended(v, size, N, g) == D.coeff_to_extended([v] * size, N, g), (g, v, size)


def test_plan_model():
    assert D.plan(1, 1) == dict(passes=0, E=0, skipped=0, rows=1, fwd_scratch=0, inv_scratch=0, plan=[])
    p = D.plan(1 << 20, 1 << 22)
    assert (p["passes"], p["E"], p["skipped"], p["rows"], p["inv_scratch"]) == (3, 2, 2, 64, 1 << 22)
    assert p["plan"] == NM.plan(22) == [(0, 8, 2), (8, 7, 3), (15, 7, 3)]
    p = D.plan((1 << 19) + 1, 1 << 22)  # not a power of two: the next one counts
    assert (p["E"], p["skipped"], p["rows"]) == (2, 2, 64)
    p = D.plan(1, 1 << 9)  # E beyond the first pass: capped at its L
    assert (p["E"], p["skipped"], p["rows"]) == (9, 5, 1)
    assert D.plan(256, 256)["inv_scratch"] == 0 and D.plan(3, 512)["inv_scratch"] == 512
