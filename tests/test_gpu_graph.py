"""The Fr graph evaluator (mbls_fr_eval_graph) on the GPU against the pure-Python interpreter of
tests/graph_model.py.  Every comparison is exact equality of the element words.  Sizes are the seams
of the 64-row tile and of the rotation wrap, not workload sizes.  The operand pool is the one of
tests/test_gpu_expr.py: every column is a window of it."""
import numpy as np
import pytest

import expr_model as E
import graph_model as G
import test_gpu_expr as X
from test_gpu_expr import amd  # noqa: F401  (the module fixture: the loaded binding)

pytestmark = pytest.mark.gpu

TILE = 64
SIZES = (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 1000)
words, ints, dev, host, column, CONSTS = X.words, X.ints, X.dev, X.host, X.column, X.CONSTS
val, col, const, NO = G.val, G.col, G.const, G.NO


def emit(src, c=0):
    return (G.EMIT, src, NO, c)


def run_gpu(amd, cols, prog, consts=(), n_outputs=1, rot_stride=1, on_device=True):
    n = len(cols[0])
    place = dev if on_device else (lambda a: a)
    got = amd.eval_graph([place(words(c)) for c in cols], prog, constants=place(words(consts)) if consts else None,
                         n_outputs=n_outputs, rot_stride=rot_stride)
    got = ints(host(got) if on_device else got)
    return [got[k * n:(k + 1) * n] for k in range(n_outputs)]


def run_both(amd, cols, prog, consts=(), n_outputs=1, rot_stride=1, on_device=True):
    """(the library's outputs, the model's), both as lists of int lists"""
    return (run_gpu(amd, cols, prog, consts, n_outputs, rot_stride, on_device),
            G.run(cols, prog, consts, n_outputs, rot_stride))


def four_columns(n):
    # windows 257 apart: every pair of 0, 1, r - 1 and random operands meets somewhere
    return [column(n, 257 * k) for k in range(4)]


# value 0 waits in a slot, value 1 is the previous op's result, then a column at a rotation and a constant
PRELUDE = [(G.STORE, col(0, 1), NO, 0), (G.DOUBLE, col(1), NO, 0)]
SOURCES = {"slot": val(0), "prev": val(1), "column": col(2, -1), "const": const(3)}
UNARY = {"square": G.SQUARE, "double": G.DOUBLE, "neg": G.NEG, "store": G.STORE}
BINARY = {"add": G.ADD, "sub": G.SUB, "mul": G.MUL, "horner": G.HORNER}


@pytest.mark.parametrize("name", sorted(UNARY) + sorted(BINARY) + ["emit"])
def test_every_opcode_alone_with_every_source_kind(amd, name):
    progs = {}
    for ka, a in SOURCES.items():
        if name == "emit":
            progs[ka] = PRELUDE + [emit(a)]
        elif name in UNARY:
            progs[ka] = PRELUDE + [(UNARY[name], a, NO, 0), emit(val(2))]
        else:
            for kb, b in SOURCES.items():
                progs[ka, kb] = PRELUDE + [(BINARY[name], a, b, 4), emit(val(2))]
    for n in SIZES:
        cols = four_columns(n)
        for key, prog in progs.items():
            got, want = run_both(amd, cols, prog, CONSTS)
            assert got == want, (n, key)
            assert all(v < E.R for v in got[0]), (n, key)


def test_one_value_as_both_operands(amd):
    for n in SIZES:
        cols = four_columns(n)
        for filler in ([], [(G.NEG, col(3), NO, 0)]):  # forwarded twice; read twice from its slot
            k = len(filler)
            prog = [(G.ADD, col(0), col(1, 1), 0)] + filler + [(G.MUL, val(0), val(0), 0), (G.SUB, val(k + 1), val(k + 1), 0),
                                                                emit(val(k + 1), 0), emit(val(k + 2), 1)]
            got, want = run_both(amd, cols, prog, n_outputs=2)
            assert got == want, (n, k)
            assert not any(got[1]), (n, k)


def test_forwarding(amd):
    c = [col(k) for k in range(4)]
    progs = {
        "as_a": [(G.ADD, c[0], c[1], 0), (G.SUB, val(0), c[2], 0), emit(val(1))],
        "as_b": [(G.ADD, c[0], c[1], 0), (G.SUB, c[2], val(0), 0), emit(val(1))],
        "as_both": [(G.ADD, c[0], c[1], 0), (G.MUL, val(0), val(0), 0), emit(val(1))],
        "and_read_later_as_a": [(G.ADD, c[0], c[1], 0), (G.SUB, val(0), c[2], 0), (G.MUL, val(0), val(1), 0), emit(val(2))],
        "and_read_later_as_b": [(G.ADD, c[0], c[1], 0), (G.SUB, c[2], val(0), 0), (G.NEG, c[3], NO, 0),
                                (G.HORNER, val(2), val(0), 3), (G.SUB, val(3), val(1), 0), emit(val(4))],
        "across_an_emit": [(G.ADD, c[0], c[1], 0), emit(c[2], 1), (G.SUB, val(0), c[3], 0), emit(val(2))],
        "a_chain": [(G.MUL, c[0], c[1], 0)] + [(op, val(k), c[k % 4], 0) for k, op in enumerate([G.ADD, G.MUL, G.SUB] * 5)] +
                   [emit(val(15))],
    }
    assert G.check(progs["a_chain"], 4, 6, 1)["peak"] == 0  # no LDS at all
    for n in SIZES:
        cols = four_columns(n)
        for name, prog in progs.items():
            nout = 2 if name == "across_an_emit" else 1
            got, want = run_both(amd, cols, prog, CONSTS, nout)
            assert got == want, (n, name)


def test_a_dead_value_changes_nothing(amd):
    n = 2 * TILE + 3
    cols = four_columns(n)
    base = [(G.MUL, col(0), col(1), 0), (G.ADD, val(0), col(2), 0), emit(val(1))]
    dead = [(G.MUL, col(0), col(1), 0), (G.SQUARE, col(3), NO, 0), (G.ADD, val(0), col(2), 0), emit(val(2))]
    assert G.check(dead, 4, 0, 1)["resident"] == 1  # the MUL's result now waits, the SQUARE's goes nowhere
    got, want = run_both(amd, cols, dead)
    assert got == want and got == run_gpu(amd, cols, base)


@pytest.mark.parametrize("stride", [1, 4])
def test_rotations_read_the_right_row(amd, stride):
    """element i encodes i: a wrong row shows as a wrong index; rows fewer than the rotation wrap twice"""
    for size in (1, 2, 3, 5, TILE - 1, TILE + 1, 1000):
        idx = [E.mont(i) for i in range(size)]
        other = column(size, 77)
        for rot in (1, -1, 3, -3):
            prog = [emit(col(0, rot), 0), (G.SUB, col(0, rot), col(1, -rot), 0), emit(val(1), 1),
                    (G.STORE, col(0, -rot), NO, 0), (G.NEG, col(1), NO, 0), (G.ADD, val(4), val(3), 0), emit(val(5), 2)]
            got, want = run_both(amd, [idx, other], prog, n_outputs=3, rot_stride=stride)
            assert got == want, (size, rot)
            assert got[0] == [E.mont((i + rot * stride) % size) for i in range(size)], (size, rot)


def test_permutation_equals_the_model_and_the_stack_evaluator(amd):
    m = 3
    for n in (TILE + 1, 1000):
        cols, consts = X.perm_inputs(m, n)
        got, want = run_both(amd, cols, G.permutation(m), consts, n_outputs=2)
        assert got == want
        dcols, dconsts = [dev(words(c)) for c in cols], dev(words(consts))
        graph = amd.eval_graph(dcols, G.permutation(m), constants=dconsts, n_outputs=2)
        lifted = amd.eval_graph(dcols, G.from_stack(E.permutation(m)), constants=dconsts, n_outputs=2)
        stack = amd.eval_program(dcols, E.permutation(m), constants=dconsts, n_outputs=2)
        assert np.array_equal(host(graph), host(stack)) and np.array_equal(host(lifted), host(stack))


def test_shared_gates(amd):
    ns, nc = 6, 8
    for n in (TILE - 1, 2 * TILE + 3):
        cols = [column(n, 43 * k + 2) for k in range(ns + 1 + nc)]
        got, want = run_both(amd, cols, G.shared_gates(ns, nc), [CONSTS[3]])
        assert got == want
        stack = amd.eval_program([dev(words(c)) for c in cols], G.shared_gates_stack(ns, nc), constants=dev(words([CONSTS[3]])))
        assert ints(host(stack)) == want[0]


def test_at_budget_uses_every_slot(amd):
    budget = amd.graph_check(G.at_budget(1), 4, 0, 1)["budget"]
    full = G.at_budget(budget)
    assert amd.graph_check(full, 4, 0, 1)["peak"] == budget
    assert sorted(s for s in G.assign_slots(full) if s is not None) == list(range(budget))
    for n in SIZES:
        got, want = run_both(amd, four_columns(n), full)
        assert got == want, n
    # the slot file filled and emptied three times over, and a shallow graph of the same values
    n = 2 * TILE + 3
    for prog in (G.at_budget(budget, 3 * budget + 5), G.at_budget(4, budget), G.at_budget(1, 9)):
        got, want = run_both(amd, four_columns(n), prog)
        assert got == want


def test_slots_are_freed_and_reused(amd):
    n = TILE + 1
    prog = G.random_graph(1, 2000, 6, 4, 2, 3, 3)
    info = amd.graph_check(prog, 6, 4, 2)
    assert info["resident"] > 200 and info["peak"] <= 3
    cols = [column(n, 61 * k + 5) for k in range(6)]
    got, want = run_both(amd, cols, prog, CONSTS[:4], n_outputs=2)
    assert got == want


def test_random_graphs(amd):
    n = 257
    cols = [column(n, 61 * k + 5) for k in range(6)]
    peaks = set()
    for seed in range(20):
        reach = (1, 2, 4, 8, 32)[seed % 5]
        prog = G.random_graph(100 + seed, 300, 6, 6, 2, 3, reach)
        peaks.add(G.check(prog, 6, 6, 2)["peak"])
        got, want = run_both(amd, cols, prog, CONSTS, n_outputs=2, rot_stride=1 + seed % 2 * 3)
        assert got == want, seed
    assert min(peaks) == 0 and max(peaks) >= 8


def test_host_columns_and_outputs(amd):
    n = 2 * TILE + 3
    prog = G.shared_gates(3, 4)
    cols, consts = [column(n, 43 * k + 2) for k in range(8)], [CONSTS[3]]
    d_out, want = run_both(amd, cols, prog, consts)
    h_out, _ = run_both(amd, cols, prog, consts, on_device=False)
    assert d_out == want and h_out == want
    # device columns, host constants, host output; and the reverse
    mixed = amd.eval_graph([dev(words(c)) for c in cols], prog, constants=words(consts), out=np.zeros((n, 4), dtype=np.uint64))
    assert ints(mixed) == want[0]
    mixed = amd.eval_graph([words(c) for c in cols], prog, constants=dev(words(consts)), out=amd.torch_u64((n, 4)))
    assert ints(host(mixed)) == want[0]


def test_async_call_and_a_dependent_call_on_one_side_stream(amd):
    import torch
    m, n = 3, 2 * TILE + 3
    cols, consts = X.perm_inputs(m, n)
    first = G.permutation(m)
    second = [(G.MUL, col(0, 1), col(1, -1), 0), (G.HORNER, val(0), col(2), m), emit(val(1))]  # num, den, v_0
    want1 = G.run(cols, first, consts, 2)
    want2 = G.run([want1[0], want1[1], cols[0]], second, consts)
    dcols, dconsts = [dev(words(c)) for c in cols], dev(words(consts))
    out1, out2 = amd.torch_u64((2 * n, 4)), amd.torch_u64((n, 4))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    amd.eval_graph(dcols, first, constants=dconsts, n_outputs=2, out=out1, stream=st, is_async=True)
    amd.eval_graph([out1[:n], out1[n:], dcols[0]], second, constants=dconsts, out=out2, stream=st, is_async=True)
    st.synchronize()
    assert ints(host(out1)) == want1[0] + want1[1]
    assert ints(host(out2)) == want2[0]
    amd.release_stream(st)


def test_errors_leave_the_output_untouched(amd):
    n = 257
    c = dev(words(column(n, 0)))
    fill = np.full((n, 4), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    out = dev(fill)
    with pytest.raises(amd.IcicleError) as e:
        amd.eval_graph([c] * 4, G.at_budget(G.BUDGET + 1), out=out)
    assert e.value.code == amd.INVALID_ARGUMENT
    assert np.array_equal(host(out), fill)
    amd.eval_graph([c], [emit(col(0))], out=out)
    assert np.array_equal(host(out), host(c))


def test_no_allocation_on_a_second_call(amd):
    n = 2 * TILE + 3
    prog = G.at_budget(G.BUDGET)
    cols = four_columns(n)
    dcols, out, hcols = [dev(words(c)) for c in cols], amd.torch_u64((n, 4)), [words(c) for c in cols]

    def calls():
        amd.eval_graph(dcols, prog, out=out)
        amd.eval_graph(hcols, prog)  # staged: the largest footprint

    calls()
    mallocs = amd.scratch_stats()[0]
    calls()
    assert amd.scratch_stats()[0] == mallocs
