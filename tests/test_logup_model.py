"""CPU-only: the model of the log-derivative lookup entries (tests/logup_model.py) against brute
force on small random cases, its counting invariant, the log-derivative identity it exists for, and
the additive operator in the tiled scan scheme at toy geometry."""
import random

import pytest

import logup_model as M
import scan_model as S

G1 = S.Geometry(K=4, wave=4, waves=2, tpg=1, agg_k=2)
G2 = G1._replace(tpg=2)


def _case(rnd, n, k, values, absent=0):
    """a table of n rows drawn from `values` distinct field values (duplicates when values < n), k
    input columns drawn from the table, `absent` cells replaced by values the table lacks"""
    pool = [M.mont(rnd.randrange(M.R)) for _ in range(values)]
    table = [rnd.choice(pool) for _ in range(n)]
    inputs = [[rnd.choice(table) for _ in range(n)] for _ in range(k)]
    have = set(table)
    for _ in range(absent):
        v = M.mont(rnd.randrange(M.R))
        while v in have:
            v = M.mont(rnd.randrange(M.R))
        inputs[rnd.randrange(k)][rnd.randrange(n)] = v
    return inputs, table


@pytest.mark.parametrize("credit", ["first", "last"])
def test_join_equals_brute_force(credit):
    rnd = random.Random(5)
    for trial in range(40):
        n, k = rnd.randrange(1, 24), rnd.randrange(1, 4)
        inputs, table = _case(rnd, n, k, rnd.randrange(1, n + 1), absent=rnd.randrange(0, 3))
        got = M.multiplicities_ref(inputs, table, credit)
        assert got == M.multiplicities_brute(inputs, table, credit), trial
        counts, missing = got
        assert sum(counts) + missing == k * n, trial
        # uncredited rows of a duplicated value read zero, and the two rules move the count only
        first, _ = M.multiplicities_ref(inputs, table, "first")
        last, _ = M.multiplicities_ref(inputs, table, "last")
        assert sum(first) == sum(last) and sorted(c for c in first if c) == sorted(c for c in last if c)


def test_missing_cells_are_counted_per_cell():
    table = [M.mont(v) for v in (3, 5, 3, 9)]
    inputs = [[M.mont(v) for v in (3, 3, 7, 7)], [M.mont(v) for v in (9, 4, 5, 3)]]
    assert M.multiplicities_ref(inputs, table, "first") == ([3, 1, 0, 1], 3)
    assert M.multiplicities_ref(inputs, table, "last") == ([0, 1, 3, 1], 3)


@pytest.mark.parametrize("credit", ["first", "last"])
def test_log_derivative_identity(credit):
    """sum_i sum_c 1 / (f_c[i] + beta) == sum_j m[j] / (t[j] + beta) when nothing is missing, with
    duplicated table values: the running sum from zero ends at zero"""
    rnd = random.Random(8)
    for trial in range(10):
        n, k = rnd.randrange(1, 20), rnd.randrange(1, 5)
        inputs, table = _case(rnd, n, k, max(1, n // 2))
        beta = M.mont(rnd.randrange(M.R))
        counts, missing = M.multiplicities_ref(inputs, table, credit)
        assert missing == 0
        m = M.count_elements(counts)
        lhs = sum(M.minv((v + beta) % M.R) for col in inputs for v in col) % M.R
        rhs = sum(M.mmul(mj, M.minv((t + beta) % M.R)) for mj, t in zip(m, table)) % M.R
        assert lhs == rhs, trial
        phi, total = M.logup_sum_ref(inputs, table, m, beta)
        assert phi[0] == 0 and total == 0, trial
        # one cell the table lacks: the sum no longer closes
        bad = [list(c) for c in inputs]
        bad[0][0] = next(v for v in (M.mont(rnd.randrange(M.R)) for _ in range(9)) if v not in table)
        counts, missing = M.multiplicities_ref(bad, table, credit)
        assert missing == 1
        assert M.logup_sum_ref(bad, table, M.count_elements(counts), beta)[1] != 0, trial


def test_terms_take_zero_for_the_inverse_of_zero():
    beta = M.mont(11)
    nb = (M.R - beta) % M.R  # the value whose denominator is zero
    table = [nb, M.mont(2)]
    inputs = [[M.mont(2), nb], [nb, nb]]
    m = [M.mont(3), M.mont(1)]
    t = M.terms_ref(inputs, table, m, beta)
    inv = M.minv((M.mont(2) + beta) % M.R)
    assert t == [inv, (0 - inv) % M.R]
    assert M.count_elements([0, 5], montgomery=False) == [0, 5]


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("g", [G1, G2], ids=["one_tile_spans", "two_tile_spans"])
def test_tiled_sum_equals_the_loop(g, inclusive):
    t, span = S.tile_elems(g), g.tpg * S.tile_elems(g)
    for n in sorted({1, 2, g.K - 1, g.K, g.K + 1, t - 1, t, t + 1, span - 1, span, span + 1, 2 * span + 3}):
        rnd = random.Random(n)
        col = [M.mont(rnd.choice([0, 1, M.R - 1] + [rnd.randrange(M.R)] * 9)) for _ in range(n)]
        init = M.mont(rnd.randrange(M.R))
        assert S.tiled_scan(M.ADD, col, g, init=init, inclusive=inclusive) == M.prefix_sum_ref(col, init, inclusive), n
        wrap = [M.R - 1] * n  # every addition wraps
        assert S.tiled_scan(M.ADD, wrap, g, inclusive=inclusive) == M.prefix_sum_ref(wrap, 0, inclusive), n
