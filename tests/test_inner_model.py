"""The model of the Fr inner products (tests/inner_model.py) against plain Horner evaluation and the
scan model's evaluation, at the edge values, and the blocked, deferred-reduction scheme of the
kernels against the plain sums at toy geometries, with the 64-bit bound of its accumulators driven
by maximal operands."""
import random

import inner_model as M
import scan_model as S

RND = random.Random(415)
R = M.R


def rand_col(n, rnd=RND):
    return [M.mont(rnd.choice([0, 1, R - 1] + [rnd.randrange(R) for _ in range(5)])) for _ in range(n)]


def horner_std(coeffs_std, z_std):
    run = 0
    for a in reversed(coeffs_std):
        run = (a + z_std * run) % R
    return run


def test_multi_eval_is_horner_and_the_scan_models_evaluation():
    cols = [rand_col(37), rand_col(37), [M.mont(5)] * 37]
    points = [0, M.ONE, M.mont(R - 1), M.mont(RND.randrange(2, R))]
    got = M.multi_eval_ref(cols, points)
    for p, c in enumerate(cols):
        std = [M.pr.fr_from_mont(a) for a in c]
        for k, z in enumerate(points):
            assert got[p * len(points) + k] == M.mont(horner_std(std, M.pr.fr_from_mont(z)))
            assert got[p * len(points) + k] == S.divide_ref(c, z)[1]


def test_zero_to_the_zero_is_one():
    col = rand_col(9)
    assert M.multi_eval_ref([col], [0]) == [col[0]]
    assert M.powers_ref(0, 4) == [M.ONE, 0, 0, 0]
    assert M.powers_ref(0, 1) == [M.ONE]
    init = M.mont(77)
    assert M.powers_ref(0, 3, init) == [init, 0, 0]
    assert M.powers_split(0, 5, init) == [init, 0, 0, 0, 0]


def test_powers_of_one_and_of_a_random_base():
    init = M.mont(RND.randrange(1, R))
    assert M.powers_ref(M.ONE, 6) == [M.ONE] * 6
    assert M.powers_ref(M.ONE, 6, init) == [init] * 6
    z = M.mont(RND.randrange(2, R))
    zs = M.pr.fr_from_mont(z)
    assert M.powers_ref(z, 20) == [M.mont(pow(zs, i, R)) for i in range(20)]


def test_the_two_table_split_is_the_running_product():
    z, init = M.mont(RND.randrange(2, R)), M.mont(RND.randrange(1, R))
    for n in (1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 100):
        assert M.powers_split(z, n, init) == M.powers_ref(z, n, init), n
        assert 1 << (2 * M.pow_log(n)) >= n
    for s in (0, 1, 3, 7):
        assert M.powers_split(z, 50, init, s) == M.powers_ref(z, 50, init), s


def test_inner_products_index_order():
    cols, vecs = [rand_col(11) for _ in range(3)], [rand_col(11) for _ in range(2)]
    got = M.inner_products_ref(cols, vecs)
    for p in range(3):
        for k in range(2):
            want = 0
            for a, b in zip(cols[p], vecs[k]):
                want = (want + M.mmul(a, b)) % R
            assert got[p * 2 + k] == want


def test_blocked_scheme_equals_the_plain_sums():
    for g in (M.Geometry(4, 7, 2, 2, 1), M.Geometry(2, 3, 2, 3, 2), M.Geometry(3, 7, 1, 1, 3)):
        tile = g.threads * g.defer
        for n in (1, 2, tile - 1, tile, tile + 1, 3 * tile + 5):
            for nc, nv in ((1, 1), (g.CB + 1, g.VB + 1)):
                cols, vecs = [rand_col(n) for _ in range(nc)], [rand_col(n) for _ in range(nv)]
                assert M.blocked_inner(cols, vecs, g) == M.inner_products_ref(cols, vecs), (g, n, nc, nv)


def test_deferred_columns_at_all_r_minus_one_operands():
    """every stored word pattern r - 1: seven maximal canonical products in every accumulator"""
    g = M.Geometry(2, M.DEFER, 2, 2, 1)
    n = 3 * g.threads * g.defer + 1
    cols, vecs, stats = [[R - 1] * n] * 3, [[R - 1] * n] * 3, {}
    assert M.blocked_inner(cols, vecs, g, stats) == M.inner_products_ref(cols, vecs)
    one = [0] * M.NCOL
    M.mac_columns(one, M.unpack29(R - 1), M.unpack29(R - 1))
    assert stats["most"] == M.DEFER and stats["peak"] == M.DEFER * max(one) < 1 << 64


def test_the_bound_is_tight_for_word_operands():
    """limbs all ones (any word operand is accepted by the unpacking): 7 products fit, 8 do not"""
    top = M.unpack29((1 << 256) - 1)
    acc = [0] * M.NCOL
    for _ in range(M.DEFER):
        M.mac_columns(acc, [M.MASK] * M.NL, [M.MASK] * M.NL)
    assert max(acc) == M.DEFER * M.COLUMN_BOUND < 1 << 64
    assert (M.DEFER + 1) * M.COLUMN_BOUND >= 1 << 64
    assert top[M.NL - 1] < 1 << 24 and all(l == M.MASK for l in top[:-1])
