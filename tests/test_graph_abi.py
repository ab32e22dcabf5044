"""CPU-only: the graph evaluator's entries are declared in the header, exported by the built library
and listed in the binding; mbls_fr_graph_op is 32 bytes on both sides; mbls_fr_graph_check, which
does no device work, agrees with the model's validator (tests/graph_model.py) in all eight numbers on
the builders, on 200 seeded random graphs and on the stack model's programs, and refuses every
malformed program of tests/test_graph_model.py; mbls_fr_eval_graph refuses before any device work.
The host lowering also runs as a stand-alone program (tests/graph_host.cpp) under
-fsanitize=address,undefined, which replays every slot assignment and whose slots are compared with
the model's."""
import ctypes
import os
import random
import subprocess

import pytest

import expr_model as E
import graph_model as G
import helpers as H
import test_abi as A
import test_graph_model as T

NAMES = {"mbls_fr_eval_graph": 11, "mbls_fr_graph_check": 6}

built = A.built  # the module fixture that builds the library when it is missing


def both(amd, prog, ncol, ncon, nout):
    want = G.check(prog, ncol, ncon, nout)
    assert amd.graph_check(prog, ncol, ncon, nout) == want
    return want


def test_header_library_and_binding_agree(built):
    fns = A.header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    amd = A._amd()
    L = amd.lib()
    for name, nargs in NAMES.items():
        assert name in fns and name in exported and name in amd.EXPORTED, name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert callable(amd.eval_graph) and callable(amd.graph_check)
    ops = [amd.GRAPH_ADD, amd.GRAPH_SUB, amd.GRAPH_MUL, amd.GRAPH_SQUARE, amd.GRAPH_DOUBLE, amd.GRAPH_NEG, amd.GRAPH_HORNER,
           amd.GRAPH_STORE, amd.GRAPH_EMIT]
    assert ops == [G.ADD, G.SUB, G.MUL, G.SQUARE, G.DOUBLE, G.NEG, G.HORNER, G.STORE, G.EMIT] == list(range(9))
    assert [amd.GRAPH_NONE, amd.GRAPH_VALUE, amd.GRAPH_COLUMN, amd.GRAPH_CONST] == [G.NONE, G.VALUE, G.COLUMN, G.CONST]
    assert amd.GRAPH_CHECK_FIELDS == G.FIELDS


def test_op_is_32_bytes_on_both_sides(tmp_path):
    amd = A._amd()
    probe = tmp_path / "probe.c"
    probe.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "bls12_381_mi355x.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mbls_fr_graph_op), sizeof(mbls_fr_graph_src), offsetof(mbls_fr_graph_op, a),
         offsetof(mbls_fr_graph_op, b), offsetof(mbls_fr_graph_op, c), offsetof(mbls_fr_graph_src, rot));
  printf("%d %d %d %d %d\n", MBLS_GRAPH_ADD, MBLS_GRAPH_HORNER, MBLS_GRAPH_EMIT, MBLS_GRAPH_NONE, MBLS_GRAPH_CONST);
  return 0;
}
''')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.dirname(A.HEADER), str(probe), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    assert lines[0].split() == ["32", "12", "4", "16", "28", "8"]
    assert lines[0].split() == [str(x) for x in (ctypes.sizeof(amd.GraphOp), ctypes.sizeof(amd.GraphSrc), amd.GraphOp.a.offset,
                                                 amd.GraphOp.b.offset, amd.GraphOp.c.offset, amd.GraphSrc.rot.offset)]
    assert lines[1].split() == [str(x) for x in (G.ADD, G.HORNER, G.EMIT, G.NONE, G.CONST)]


@pytest.mark.parametrize("name", sorted(T.VALID))
def test_check_numbers_equal_the_models(built, name):
    both(A._amd(), *T.VALID[name])


@pytest.mark.parametrize("name", sorted(T.STACK))
def test_check_numbers_of_stack_programs_as_graphs(built, name):
    prog, ncol, ncon, nout = T.STACK[name]
    both(A._amd(), G.from_stack(prog), ncol, ncon, nout)


def random_case(seed):
    rnd = random.Random(1000 + seed)
    reach, nout, ncon = rnd.choice([1, 2, 3, 8, 20, 32]), rnd.randint(1, 8), rnd.choice([0, 1, 5])
    return G.random_graph(seed, rnd.randint(2 * nout, 400), rnd.randint(1, 9), ncon, nout, rnd.randint(0, 4), reach), ncon, nout


def test_check_numbers_of_200_random_graphs(built):
    amd = A._amd()
    peaks = set()
    for seed in range(200):
        prog, ncon, nout = random_case(seed)
        peaks.add(both(amd, prog, 9, ncon, nout)["peak"])
    assert 0 in peaks and max(peaks) >= 8  # the seeds cover shallow and deep graphs


@pytest.mark.parametrize("name", sorted(T.MALFORMED))
def test_check_refuses_what_the_model_refuses(built, name):
    amd = A._amd()
    prog, ncol, ncon, nout = T.MALFORMED[name]
    with pytest.raises(G.ProgramError):
        G.check(prog, ncol, ncon, nout)
    with pytest.raises(amd.IcicleError) as e:
        amd.graph_check(prog, ncol, ncon, nout)
    assert e.value.code == amd.INVALID_ARGUMENT


def test_budget_is_the_last_peak_accepted(built):
    amd = A._amd()
    budget = amd.graph_check(G.at_budget(1), 4, 0, 1)["budget"]
    assert budget == G.BUDGET and budget >= 32
    info = both(amd, G.at_budget(budget), 4, 0, 1)
    assert info["peak"] == budget and info["peak_at"] == budget
    with pytest.raises(amd.IcicleError) as e:
        amd.graph_check(G.at_budget(budget + 1), 4, 0, 1)
    assert e.value.code == amd.INVALID_ARGUMENT
    # refused for its peak alone: the numbers say where to cut
    with pytest.raises(G.ProgramError) as m:
        G.check(G.at_budget(budget + 1), 4, 0, 1)
    assert e.value.info == m.value.info and e.value.info["peak"] == budget + 1 and e.value.info["peak_at"] == budget + 1
    # refused for another rule: nothing is written
    with pytest.raises(amd.IcicleError) as e:
        amd.graph_check(*T.MALFORMED["output_twice"])
    assert not hasattr(e.value, "info")


def test_forwarded_and_resident_counts(built):
    amd = A._amd()
    c0, val, NO, X = G.col(0), G.val, G.NO, T.X
    only_next = [(G.NEG, c0, NO, 0), (G.NEG, val(0), NO, 0), X(val(1))]
    info = both(amd, only_next, 1, 0, 1)
    assert (info["forwarded"], info["resident"], info["peak"]) == (2, 0, 0)
    next_and_later = [(G.NEG, c0, NO, 0), (G.NEG, val(0), NO, 0), (G.ADD, val(1), val(0), 0), X(val(2))]
    info = both(amd, next_and_later, 1, 0, 1)
    assert (info["forwarded"], info["resident"], info["peak"], info["peak_at"]) == (3, 1, 1, 1)
    dead = [(G.SQUARE, c0, NO, 0), (G.NEG, c0, NO, 0), X(val(1))]
    info = both(amd, dead, 1, 0, 1)
    assert (info["forwarded"], info["resident"], info["peak"]) == (1, 0, 0)


def test_check_null_pointers(built):
    amd = A._amd()
    L = amd.lib()
    ops = amd._graph_program([(G.NEG, G.col(0), G.NO, 0), T.X(G.val(0))])
    out = (ctypes.c_int32 * 8)()
    assert L.mbls_fr_graph_check(None, 2, 1, 0, 1, out) == amd.INVALID_POINTER
    assert L.mbls_fr_graph_check(ops, 2, 1, 0, 1, None) == amd.INVALID_POINTER
    assert L.mbls_fr_graph_check(ops, 2, 1, 0, 1, out) == amd.SUCCESS and list(out) == [0, 0, 0, 1, 1, 1, 0, G.BUDGET]


def test_eval_graph_refuses_before_any_device_work(built):
    """every refusal of mbls_fr_eval_graph comes before the first HIP call, so it answers here too"""
    amd = A._amd()
    L = amd.lib()
    col = (ctypes.c_uint64 * 8)()
    table = (ctypes.c_void_p * 2)(ctypes.addressof(col), ctypes.addressof(col))
    holed = (ctypes.c_void_p * 2)(ctypes.addressof(col), None)
    full = (ctypes.c_void_p * 1025)(*[ctypes.addressof(col)] * 1025)
    full[1023] = None
    ok = amd._graph_program([(G.NEG, G.col(1), G.NO, 0), T.X(G.val(0))])
    deep_prog = G.at_budget(G.BUDGET + 1)
    deep = amd._graph_program(deep_prog)
    cfg = ctypes.byref(amd.vec_config())
    out = (ctypes.c_uint64 * 8)()
    P, A_ = amd.INVALID_POINTER, amd.INVALID_ARGUMENT
    f = L.mbls_fr_eval_graph
    cases = [
        (f(None, 2, 2, 1, None, 0, ok, 2, 1, cfg, out), P),
        (f(table, 2, 2, 1, None, 0, None, 2, 1, cfg, out), P),
        (f(table, 2, 2, 1, None, 0, ok, 2, 1, None, out), P),
        (f(table, 2, 2, 1, None, 0, ok, 2, 1, cfg, None), P),
        (f(table, 2, 2, 1, None, 1, ok, 2, 1, cfg, out), P),
        (f(holed, 2, 2, 1, None, 0, ok, 2, 1, cfg, out), P),
        (f(table, 2, 0, 1, None, 0, ok, 2, 1, cfg, out), A_),
        (f(table, 2, (1 << 26) + 1, 1, None, 0, ok, 2, 1, cfg, out), A_),
        (f(table, 2, 2, 0, None, 0, ok, 2, 1, cfg, out), A_),
        (f(table, 2, 2, (1 << 26) + 1, None, 0, ok, 2, 1, cfg, out), A_),
        (f(table, 1, 2, 1, None, 0, ok, 2, 1, cfg, out), A_),  # column 1 of 1
        (f(table, 2, 2, 1, None, 0, deep, len(deep_prog), 1, cfg, out), A_),  # column 3 of 2
        (f((ctypes.c_void_p * 4)(*[ctypes.addressof(col)] * 4), 4, 2, 1, None, 0, deep, len(deep_prog), 1, cfg, out), A_),
        # a table of the most columns whose last is null: alone, then with a malformed program, no
        # rows, one column too many -- the program, the size and the count are looked at first
        (f(full, 1024, 2, 1, None, 0, ok, 2, 1, cfg, out), P),
        (f(full, 1024, 2, 1, None, 0, deep, len(deep_prog), 1, cfg, out), A_),
        (f(full, 1024, 0, 1, None, 0, ok, 2, 1, cfg, out), A_),
        (f(full, 1025, 2, 1, None, 0, ok, 2, 1, cfg, out), A_),
    ]
    for k, (got, want) in enumerate(cases):
        assert got == want, k
    assert not any(out)


# ----------------------------------------------------------------------------- the lowering under the sanitizers
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("graph") / "graph_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd", "csrc"), "-I", os.path.join(H.ROOT, "include"),
                           os.path.join(H.ROOT, "tests", "graph_host.cpp"), "-o", str(exe)])

    def lower(cases):
        """[(code, numbers or None, put slots or None, operand sources or None)] per (prog, ncol, ncon, nout)"""
        text = []
        for prog, ncol, ncon, nout in cases:
            text.append(f"{len(prog)} {ncol} {ncon} {nout}")
            text += [" ".join(str(v) for v in (op, *a, *b, c)) for op, a, b, c in prog]
        res = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        lines, got = res.stdout.splitlines(), []
        while lines:
            head = [int(v) for v in lines.pop(0).split()]
            slots = froms = None
            if head[0] == 0:
                slots, froms = [int(v) for v in lines.pop(0).split()], lines.pop(0).split()
            got.append((head[0], head[1:] or None, slots, froms))
        assert len(got) == len(cases)
        return got
    return lower


def expected_sources(prog, slots):
    out = []
    for k, (op, a, b, c) in enumerate(prog):
        s = ""
        for kind, idx, _ in (a, b):
            s += {G.NONE: "0", G.COLUMN: "3", G.CONST: "4"}.get(kind) or ("1" if idx == k - 1 else f"2[{slots[idx]}]")
        out.append(s)
    return out


def test_lowering_under_the_sanitizers(harness):
    names = sorted(T.MALFORMED)
    for name, (code, numbers, slots, froms) in zip(names, harness([T.MALFORMED[n] for n in names])):
        assert code == 11 and slots is None, name
        assert (numbers is not None) == (name == "peak_33"), name
    valid = [T.VALID[n] for n in sorted(T.VALID)] + [(G.at_budget(b), 4, 0, 1) for b in (1, 2, 31, 32)]
    valid += [(p, 9, ncon, nout) for p, ncon, nout in map(random_case, range(40))]
    valid += [(G.random_graph(77, G.MAX_OPS, 6, 4, 8, 3, 32), 6, 4, 8)]  # the longest program, the widest reach
    for (prog, ncol, ncon, nout), (code, numbers, slots, froms) in zip(valid, harness(valid)):
        want = G.check(prog, ncol, ncon, nout)
        assert code == 0 and numbers == [want[f] for f in G.FIELDS]
        model = G.assign_slots(prog)
        assert slots == [-1 if s is None else s for s in model]
        assert froms == expected_sources(prog, model)
