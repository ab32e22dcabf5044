"""CPU-only, no library: the expression model (tests/expr_model.py) against closed formulas written
independently as list comprehensions over canonical integers, its rotation wrap, and its validator
on one malformed program per rule."""
import random

import pytest

import expr_model as E

R = E.R
RINV = E.S.pr.FR_RINV


def canon(col):
    return [x * RINV % R for x in col]


def column(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)]


def mcol(col):
    return [E.mont(x) for x in col]


def test_permutation_is_the_product_of_its_factors():
    m, n = 3, 11
    v = [column(n, k) for k in range(m)]
    sg = [column(n, 10 + k) for k in range(m)]
    x = column(n, 20)
    beta, gamma, delta = 5, 7, 11
    consts = [beta * pow(delta, k, R) % R for k in range(m)] + [beta, gamma]
    out = E.run([mcol(c) for c in v + sg + [x]], E.permutation(m), mcol(consts), n_outputs=2)
    num, den = [1] * n, [1] * n
    for k in range(m):
        num = [num[i] * (v[k][i] + beta * pow(delta, k, R) * x[i] + gamma) % R for i in range(n)]
        den = [den[i] * (v[k][i] + beta * sg[k][i] + gamma) % R for i in range(n)]
    assert [canon(o) for o in out] == [num, den]
    assert E.check(E.permutation(m), 2 * m + 1, m + 2, 2) == dict(depth=3, loads=4 * m, muls=4 * m - 2, pairs=2 * m + 1)


def test_compression_is_the_power_sum():
    m, n, theta = 5, 9, 123456789
    a = [column(n, 30 + k) for k in range(m)]
    out = E.run([mcol(c) for c in a], E.compression(m), mcol([theta]))
    assert canon(out[0]) == [sum(pow(theta, k, R) * a[k][i] for k in range(m)) % R for i in range(n)]
    assert E.check(E.compression(m), m, 1, 1)["depth"] == 2


@pytest.mark.parametrize("horner", [True, False])
def test_gate_fold_is_the_y_combination(horner):
    n, y = 13, 987654321
    q, a, b, c = (column(n, 40 + k) for k in range(4))
    out = E.run([mcol(t) for t in (q, a, b, c)], E.gate_fold(horner), mcol([y]))
    g0 = [q[i] * (a[i] * b[(i + 1) % n] - c[i]) for i in range(n)]
    g1 = [q[i] * (a[i] - c[(i - 1) % n]) for i in range(n)]
    g2 = [a[i] * a[i] - a[i] for i in range(n)]
    assert canon(out[0]) == [(g0[i] * y ** 3 + g1[i] * y ** 2 + g2[i] * y) % R for i in range(n)]


@pytest.mark.parametrize("size", [5, 12, 257])
@pytest.mark.parametrize("stride", [1, 4])
def test_rotation_wraps(size, stride):
    col = [E.mont(i) for i in range(size)]  # element i encodes i
    for b in (-(size - 1), -1, 0, 1, size - 1, size + 5, -3 * size - 2, 2 ** 31 - 1, -2 ** 31):
        out = E.run([col], [(E.COLUMN, 0, b), (E.EMIT, 0, 0)], rot_stride=stride)
        got = canon(out[0])
        assert got == [(i + b * stride) % size for i in range(size)], (b, stride)
        assert all(0 <= g < size for g in got)


def test_random_programs_are_valid_and_reach_their_depth():
    for seed, n_ops, depth, outs in ((1, 40, 1, 1), (2, 64, 2, 2), (3, 200, 8, 1), (4, 4096, 8, 1), (5, 300, 5, 8)):
        prog = E.random_program(seed, n_ops, depth, 16, 16, outs)
        info = E.check(prog, 16, 16, outs)
        assert len(prog) == n_ops and info["depth"] == depth
    assert E.random_program(9, 100, 4, 3, 2) == E.random_program(9, 100, 4, 3, 2)


C, K, A, M, X = E.COLUMN, E.CONST, E.ADD, E.MUL, E.EMIT
MALFORMED = {
    "underflow": ([(C, 0, 0), (A, 0, 0), (X, 0, 0)], 1, 1, 1),
    "unary_underflow": ([(E.NEG, 0, 0), (C, 0, 0), (X, 0, 0)], 1, 1, 1),
    "emit_underflow": ([(C, 0, 0), (X, 0, 0), (X, 1, 0)], 1, 1, 2),
    "depth_9": ([(C, 0, 0)] * 9 + [(A, 0, 0)] * 8 + [(X, 0, 0)], 1, 1, 1),
    "bad_opcode": ([(C, 0, 0), (11, 0, 0), (X, 0, 0)], 1, 1, 1),
    "negative_opcode": ([(C, 0, 0), (-1, 0, 0), (X, 0, 0)], 1, 1, 1),
    "bad_column": ([(C, 2, 0), (X, 0, 0)], 2, 1, 1),
    "negative_column": ([(C, -1, 0), (X, 0, 0)], 2, 1, 1),
    "bad_constant": ([(K, 1, 0), (X, 0, 0)], 1, 1, 1),
    "constant_without_constants": ([(C, 0, 0), (E.SCALE, 0, 0), (X, 0, 0)], 1, 0, 1),
    "bad_horner_constant": ([(C, 0, 0), (C, 0, 0), (E.HORNER, 3, 0), (X, 0, 0)], 1, 3, 1),
    "bad_output": ([(C, 0, 0), (X, 1, 0)], 1, 1, 1),
    "double_emit": ([(C, 0, 0), (X, 0, 0), (C, 0, 0), (X, 0, 0)], 1, 1, 2),
    "missing_emit": ([(C, 0, 0), (X, 0, 0)], 1, 1, 2),
    "leftover": ([(C, 0, 0), (C, 0, 0), (X, 0, 0)], 1, 1, 1),
    "n_ops_0": ([], 1, 1, 1),
    "n_ops_4097": ([(C, 0, 0), (E.NEG, 0, 0)] + [(E.NEG, 0, 0)] * 4094 + [(X, 0, 0)], 1, 1, 1),
    "n_outputs_0": ([(C, 0, 0), (X, 0, 0)], 1, 1, 0),
    "n_outputs_9": ([(C, 0, 0), (X, 0, 0)], 1, 1, 9),
    "n_columns_0": ([(K, 0, 0), (X, 0, 0)], 0, 1, 1),
    "n_columns_1025": ([(C, 0, 0), (X, 0, 0)], 1025, 1, 1),
    "n_constants_1025": ([(C, 0, 0), (X, 0, 0)], 1, 1025, 1),
}
VALID = {
    "depth_1": ([(C, 0, 0), (E.SQUARE, 0, 0), (X, 0, 0)], 1, 0, 1),
    "depth_8": ([(C, 0, k) for k in range(8)] + [(E.SUB, 0, 0)] * 7 + [(X, 0, 0)], 1, 0, 1),
    "length_4096": (E.random_program(4, 4096, 8, 16, 16), 16, 16, 1),
    "permutation": (E.permutation(3), 7, 5, 2),
    "limits": ([(C, 1023, -2 ** 31), (K, 1023, 0), (M, 0, 0), (X, 7, 0)] + [t for k in range(7) for t in ((C, 0, 2 ** 31 - 1), (X, k, 0))],
               1024, 1024, 8),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_validator_refuses(name):
    prog, ncol, ncon, nout = MALFORMED[name]
    with pytest.raises(E.ProgramError):
        E.check(prog, ncol, ncon, nout)


def test_validator_counts():
    assert len(MALFORMED["n_ops_4097"][0]) == 4097
    assert E.check(*VALID["depth_1"]) == dict(depth=1, loads=1, muls=1, pairs=1)
    assert E.check(*VALID["depth_8"]) == dict(depth=8, loads=8, muls=0, pairs=8)
    assert E.check(*VALID["limits"]) == dict(depth=2, loads=8, muls=1, pairs=2)
    info = E.check(*VALID["length_4096"])
    assert info["depth"] == 8 and info["pairs"] <= info["loads"]
