"""CPU-only, no library: the graph model (tests/graph_model.py) against the stack model it extends
(tests/expr_model.py) and against closed formulas, its residency numbers on programs small enough
to count by hand, its slot assignment, and its validator on one malformed program per rule, each
differing from a valid program in exactly that respect."""
import functools
import random

import pytest

import expr_model as E
import graph_model as G
import test_expr_model as T

R = G.R
canon, column, mcol = T.canon, T.column, T.mcol
val, col, const, NO = G.val, G.col, G.const, G.NO

# stack programs of expr_model.py with their (n_columns, n_constants, n_outputs)
STACK = {
    "permutation": (E.permutation(3), 7, 5, 2),
    "compression": (E.compression(5), 5, 1, 1),
    "gate_fold_horner": (E.gate_fold(True), 4, 1, 1),
    "gate_fold_plain": (E.gate_fold(False), 4, 1, 1),
    "random_depth_8": (E.random_program(3, 200, 8, 16, 16), 16, 16, 1),
    "random_8_outputs": (E.random_program(5, 300, 5, 16, 16, 8), 16, 16, 8),
    "random_4096": (E.random_program(4, 4096, 8, 16, 16), 16, 16, 1),
    "depth_8": T.VALID["depth_8"],
    "limits": T.VALID["limits"],
    "shared_gates_stack": (G.shared_gates_stack(6, 8), 15, 1, 1),
}


def inputs(n, n_columns, n_constants, seed=7):
    return [mcol(column(n, seed + k)) for k in range(n_columns)], mcol(column(n_constants, seed + 5000))


@pytest.mark.parametrize("name", sorted(STACK))
def test_from_stack_computes_what_the_stack_program_computes(name):
    prog, ncol, ncon, nout = STACK[name]
    g = G.from_stack(prog)
    info = G.check(g, ncol, ncon, nout)
    pushes = sum(op in (E.COLUMN, E.CONST) for op, _, _ in prog)
    assert len(g) == len(prog) - pushes
    assert info["muls"] == E.check(prog, ncol, ncon, nout)["muls"] and info["loads"] == E.check(prog, ncol, ncon, nout)["loads"]
    assert info["peak"] <= E.MAX_DEPTH
    n = 3 if len(prog) > 1000 else 7
    cols, consts = inputs(n, ncol, ncon)
    assert G.run(cols, g, consts, nout) == E.run(cols, prog, consts, nout)
    assert G.run(cols, g, consts, nout, rot_stride=4) == E.run(cols, prog, consts, nout, rot_stride=4)


def test_permutation_is_the_product_of_its_factors():
    m, n = 3, 11
    cols, consts = inputs(n, 2 * m + 1, m + 2)
    assert G.run(cols, G.permutation(m), consts, 2) == E.run(cols, E.permutation(m), consts, 2)
    # three ops per factor less the first product of each side, an EMIT per side; only the running product
    # waits in a slot
    info = G.check(G.permutation(m), 2 * m + 1, m + 2, 2)
    assert len(G.permutation(m)) == 2 * (3 * m - 1) + 2
    assert info == dict(peak=1, peak_at=2, resident=2 * (m - 1), forwarded=4 * m, loads=4 * m,
                        pairs=2 * m + 1, muls=4 * m - 2, budget=G.BUDGET)


def test_shared_gates_is_the_fold_of_its_constraints():
    ns, nc, n, y = 6, 8, 9, 987654321
    raw = [column(n, 60 + k) for k in range(ns + 1 + nc)]
    out = G.run([mcol(c) for c in raw], G.shared_gates(ns, nc), mcol([y]))
    want = []
    for i in range(n):
        s = 1
        for k in range(ns + 1):
            s = s * raw[k][i] % R
        want.append(sum(pow(y, nc - 1 - j, R) * s * raw[ns + 1 + j][(i + j % 3 - 1) % n] for j in range(nc)) % R)
    assert canon(out[0]) == want
    info = G.check(G.shared_gates(ns, nc), ns + 1 + nc, 1, 1)
    # S and the fold's accumulator wait; S is computed once
    assert info["muls"] == ns + 2 * nc - 1 and info["peak"] == 2 and info["loads"] == ns + 1 + nc
    stack = G.shared_gates_stack(ns, nc)
    assert E.check(stack, ns + 1 + nc, 1, 1)["muls"] == nc * (ns + 1) + nc - 1
    assert E.run([mcol(c) for c in raw], stack, mcol([y])) == out


@pytest.mark.parametrize("b,total", [(1, 1), (1, 5), (2, 2), (4, 32), (5, 7), (31, 31), (32, 32), (32, 70)])
def test_at_budget_has_exactly_its_peak(b, total):
    g = G.at_budget(b, total)
    info = G.check(g, G.AT_BUDGET_COLUMNS, 0, 1)
    assert len(g) == 2 * total + 2
    assert info["peak"] == b and info["peak_at"] == b
    slots = G.assign_slots(g)
    assert sorted(set(s for s in slots if s is not None)) == list(range(b))  # every slot in use, none beyond
    # the fold, written out
    n = 5
    raw = [column(n, 80 + k) for k in range(G.AT_BUDGET_COLUMNS)]
    out = G.run([mcol(c) for c in raw], g)
    x = lambda j, i: raw[j % 4][(i + j // 4) % n]
    want = []
    for i in range(n):
        acc, done = raw[0][(i - 1) % n], 0
        while done < total:
            k = min(b, total - done)
            for j in range(done + k - 1, done - 1, -1):
                acc = acc * x(j, i) % R if j % 2 == 0 else (acc - x(j, i)) % R
            done += k
        want.append(acc)
    assert canon(out[0]) == want


def test_one_past_the_budget_is_refused_and_says_where_to_cut():
    assert G.check(G.at_budget(G.BUDGET), 4, 0, 1)["peak"] == G.BUDGET
    with pytest.raises(G.ProgramError) as e:
        G.check(G.at_budget(G.BUDGET + 1), 4, 0, 1)
    assert e.value.info["peak"] == G.BUDGET + 1 and e.value.info["peak_at"] == G.BUDGET + 1


X = lambda src, c=0: (G.EMIT, src, NO, c)


def test_forwarding_and_residency_by_hand():
    c0 = col(0)
    # read by the next op only: forwarded, not resident
    info = G.check([(G.NEG, c0, NO, 0), (G.NEG, val(0), NO, 0), X(val(1))], 1, 0, 1)
    assert (info["forwarded"], info["resident"], info["peak"], info["peak_at"]) == (2, 0, 0, 0)
    # read by the next op and by a later one: forwarded once, and resident
    g = [(G.NEG, c0, NO, 0), (G.NEG, val(0), NO, 0), (G.ADD, val(1), val(0), 0), X(val(2))]
    info = G.check(g, 1, 0, 1)
    assert (info["forwarded"], info["resident"], info["peak"], info["peak_at"]) == (3, 1, 1, 1)
    assert G.assign_slots(g) == [0, None, None, None]
    # both operands of one op forwarded: two forwarded operands, nothing resident
    info = G.check([(G.NEG, c0, NO, 0), (G.MUL, val(0), val(0), 0), X(val(1))], 1, 0, 1)
    assert (info["forwarded"], info["resident"]) == (3, 0)
    # a later reader only: resident, nothing forwarded; an EMIT between does not forward
    g = [(G.NEG, c0, NO, 0), X(c0, 1), (G.NEG, val(0), NO, 0), X(val(2))]
    info = G.check(g, 1, 0, 2)
    assert (info["forwarded"], info["resident"], info["peak"], info["peak_at"]) == (1, 1, 1, 1)
    # a value nobody reads: allowed, neither resident nor forwarded
    info = G.check([(G.SQUARE, c0, NO, 0), (G.NEG, c0, NO, 0), X(val(1))], 1, 0, 1)
    assert (info["forwarded"], info["resident"], info["peak"], info["muls"]) == (1, 0, 0, 1)
    # a slot is free for the result of the op that reads its value last
    g = [(G.NEG, c0, NO, 0), (G.NEG, c0, NO, 0), (G.ADD, val(0), c0, 0), (G.NEG, c0, NO, 0), (G.ADD, val(2), val(1), 0),
         X(val(4))]
    assert G.assign_slots(g) == [0, 1, 0, None, None, None]
    assert G.check(g, 1, 0, 1)["peak"] == 2


def test_random_graphs_are_valid_and_stay_inside_their_reach():
    for seed in range(40):
        rnd = random.Random(seed)
        reach, nout, ncon = rnd.choice([1, 2, 5, 32]), rnd.randint(1, 8), rnd.choice([0, 3])
        g = G.random_graph(seed, rnd.randint(2 * nout, 300), 6, ncon, nout, 3, reach)
        info = G.check(g, 6, ncon, nout)
        assert info["peak"] <= reach
        slots = [s for s in G.assign_slots(g) if s is not None]
        assert len(slots) == info["resident"] and (max(slots) + 1 if slots else 0) == info["peak"]
    assert G.random_graph(9, 100, 3, 2, 2, 3, 8) == G.random_graph(9, 100, 3, 2, 2, 3, 8)
    big = G.random_graph(1, 2000, 6, 4, 2, 3, 3)
    assert G.check(big, 6, 4, 2)["resident"] > 200  # slots are left and taken again many times


def test_random_graph_against_a_second_interpreter():
    """run() against a recursive evaluation of the outputs' expression trees over canonical integers"""
    g = G.random_graph(11, 60, 4, 3, 2, 2, 6)
    n = 6
    raw, kraw = [column(n, 90 + k) for k in range(4)], column(3, 99)
    out = G.run([mcol(c) for c in raw], g, mcol(kraw), 2, rot_stride=2)

    @functools.lru_cache(maxsize=None)
    def ev(src, i):
        kind, idx, rot = src
        if kind == G.COLUMN:
            return raw[idx][(i + 2 * rot) % n]
        if kind == G.CONST:
            return kraw[idx]
        op, a, b, c = g[idx]
        x = ev(a, i)
        return {G.ADD: lambda: x + ev(b, i), G.SUB: lambda: x - ev(b, i), G.MUL: lambda: x * ev(b, i), G.SQUARE: lambda: x * x,
                G.DOUBLE: lambda: 2 * x, G.NEG: lambda: -x, G.HORNER: lambda: x * kraw[c] + ev(b, i), G.STORE: lambda: x}[op]() % R

    for op, a, b, c in g:
        if op == G.EMIT:
            assert canon(out[c]) == [ev(a, i) for i in range(n)]


# ----------------------------------------------------------------------------- the validator's table
NCOL, NCON, NOUT = 2, 2, 2
BASE = [(G.MUL, col(0, 1), col(1), 0),      # 0
        (G.HORNER, val(0), const(1), 1),    # 1
        (G.NEG, val(1), NO, 0),             # 2
        (G.SQUARE, val(0), NO, 0),          # 3
        (G.DOUBLE, val(3), NO, 0),          # 4
        (G.STORE, val(4), NO, 0),           # 5
        X(val(5), 1),                       # 6
        (G.ADD, val(2), const(0), 0),       # 7
        (G.SUB, val(7), col(1, -1), 0),     # 8
        X(val(8), 0)]                       # 9


def edit(k, op=None, a=None, b=None, c=None, base=BASE):
    o = base[k]
    g = list(base)
    g[k] = (o[0] if op is None else op, o[1] if a is None else a, o[2] if b is None else b, o[3] if c is None else c)
    return g


LONG = G.random_graph(2, G.MAX_OPS, 6, 4, 2, 3, 8)
MALFORMED = {
    "n_ops_0": ([], NCOL, NCON, NOUT),
    "n_ops_16385": (LONG[:-1] + [(G.NEG, col(0), NO, 0)] + LONG[-1:], 6, 4, 2),
    "n_columns_0": (BASE, 0, NCON, NOUT),
    "n_columns_1025": (BASE, 1025, NCON, NOUT),
    "n_constants_negative": (BASE, NCOL, -1, NOUT),
    "n_constants_1025": (BASE, NCOL, 1025, NOUT),
    "n_outputs_0": (BASE, NCOL, NCON, 0),
    "n_outputs_9": (BASE, NCOL, NCON, 9),
    "opcode_9": (edit(5, op=9), NCOL, NCON, NOUT),
    "opcode_negative": (edit(5, op=-1), NCOL, NCON, NOUT),
    "kind_4_in_a": (edit(2, a=(4, 1, 0)), NCOL, NCON, NOUT),
    "kind_4_in_b": (edit(7, b=(4, 0, 0)), NCOL, NCON, NOUT),
    "kind_negative": (edit(2, a=(-1, 1, 0)), NCOL, NCON, NOUT),
    "b_on_neg": (edit(2, b=col(0)), NCOL, NCON, NOUT),
    "b_on_square": (edit(3, b=val(1)), NCOL, NCON, NOUT),
    "b_on_double": (edit(4, b=const(0)), NCOL, NCON, NOUT),
    "b_on_store": (edit(5, b=col(1)), NCOL, NCON, NOUT),
    "b_on_emit": (edit(6, b=val(5)), NCOL, NCON, NOUT),
    "a_none_on_neg": (edit(2, a=NO), NCOL, NCON, NOUT),
    "a_none_on_emit": (edit(6, a=NO), NCOL, NCON, NOUT),
    "a_none_on_mul": (edit(0, a=NO), NCOL, NCON, NOUT),
    "b_none_on_mul": (edit(0, b=NO), NCOL, NCON, NOUT),
    "b_none_on_horner": (edit(1, b=NO), NCOL, NCON, NOUT),
    "b_none_on_add": (edit(7, b=NO), NCOL, NCON, NOUT),
    "b_none_on_sub": (edit(8, b=NO), NCOL, NCON, NOUT),
    "value_is_itself": (edit(2, a=val(2)), NCOL, NCON, NOUT),
    "value_is_later": (edit(2, a=val(3)), NCOL, NCON, NOUT),
    "value_negative": (edit(2, a=val(-1)), NCOL, NCON, NOUT),
    "value_is_an_emit": (edit(7, a=val(6)), NCOL, NCON, NOUT),
    "value_in_b_is_later": (edit(7, b=val(8)), NCOL, NCON, NOUT),
    "column_2_of_2": (edit(0, a=col(2, 1)), NCOL, NCON, NOUT),
    "column_negative": (edit(8, b=col(-1, -1)), NCOL, NCON, NOUT),
    "constant_2_of_2": (edit(7, b=const(2)), NCOL, NCON, NOUT),
    "constant_negative": (edit(1, b=const(-1)), NCOL, NCON, NOUT),
    "constant_without_constants": (edit(1, op=G.ADD, base=edit(7, b=col(0))), NCOL, 0, NOUT),  # op 1 still reads const(1)
    "horner_constant_2_of_2": (edit(1, c=2), NCOL, NCON, NOUT),
    "horner_constant_negative": (edit(1, c=-1), NCOL, NCON, NOUT),
    "output_2_of_2": (edit(6, c=2), NCOL, NCON, NOUT),
    "output_negative": (edit(6, c=-1), NCOL, NCON, NOUT),
    "output_twice": (edit(6, c=0), NCOL, NCON, NOUT),
    "output_never": (BASE, NCOL, NCON, 3),
    "peak_33": (G.at_budget(G.BUDGET + 1), 4, 0, 1),
}
VALID = {
    "base": (BASE, NCOL, NCON, NOUT),
    "base_without_constants": (edit(1, op=G.ADD, b=col(0), base=edit(7, b=col(0))), NCOL, 0, NOUT),
    "length_16384": (LONG, 6, 4, 2),
    "permutation": (G.permutation(3), 7, 5, 2),
    "shared_gates": (G.shared_gates(6, 8), 15, 1, 1),
    "at_budget": (G.at_budget(G.BUDGET), 4, 0, 1),
    "at_budget_long": (G.at_budget(G.BUDGET, 100), 4, 0, 1),
    "peak_4_of_32_values": (G.at_budget(4, 32), 4, 0, 1),
    "reuse_2000": (G.random_graph(1, 2000, 6, 4, 2, 3, 3), 6, 4, 2),
    "fields_that_are_not_read": ([(G.NEG, (G.CONST, 0, 99), (G.NONE, -5, 7), -3), (G.EMIT, (G.VALUE, 0, 12), NO, 0)], 1, 1, 1),
    "limits": ([(G.MUL, col(1023, -2 ** 31), const(1023), 0), (G.HORNER, val(0), col(0, 2 ** 31 - 1), 1023), X(val(1), 7)] +
               [X(col(0, k), k) for k in range(7)], 1024, 1024, 8),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_validator_refuses(name):
    prog, ncol, ncon, nout = MALFORMED[name]
    with pytest.raises(G.ProgramError):
        G.check(prog, ncol, ncon, nout)


def test_validator_accepts_and_counts():
    assert len(MALFORMED["n_ops_16385"][0]) == G.MAX_OPS + 1 and len(LONG) == G.MAX_OPS
    for name in VALID:
        G.check(*VALID[name])
    # value 0 waits for op 3, value 2 for op 7: ops 1..3 and 3..7
    assert G.check(*VALID["base"]) == dict(peak=2, peak_at=3, resident=2, forwarded=7, loads=3, pairs=3, muls=3,
                                          budget=G.BUDGET)
    assert G.check(*VALID["limits"])["pairs"] == 9
    assert G.check(*VALID["peak_4_of_32_values"])["peak"] == 4
    assert len(VALID["peak_4_of_32_values"][0]) == len(VALID["at_budget"][0])
