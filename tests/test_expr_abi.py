"""CPU-only: the expression evaluator's entries are declared in the header, exported by the built
library and listed in the binding's EXPORTED with their argument lists; mbls_fr_expr_check, which
does no device work, agrees with the model's validator (tests/expr_model.py) on a machine without a
GPU: the four counters of valid programs, INVALID_ARGUMENT for one malformed program per rule."""
import ctypes
import subprocess

import pytest

import expr_model as E
import test_abi as A
import test_expr_model as T

NAMES = {"mbls_fr_eval_program": 11, "mbls_fr_expr_check": 6}

built = A.built  # the module fixture that builds the library when it is missing


def test_header_declares_expr():
    fns = A.header_functions()
    for name in NAMES:
        assert name in fns, name


def test_library_exports_expr(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for name in NAMES:
        assert name in exported, name


def test_binding_lists_expr(built):
    amd = A._amd()
    for name in NAMES:
        assert name in amd.EXPORTED, name
    L = amd.lib()
    for name, nargs in NAMES.items():  # the binding gave each an argument list
        assert getattr(L, name).argtypes is not None, name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert callable(amd.eval_program) and callable(amd.expr_check)
    ops = [amd.EXPR_COLUMN, amd.EXPR_CONST, amd.EXPR_ADD, amd.EXPR_SUB, amd.EXPR_MUL, amd.EXPR_NEG, amd.EXPR_DOUBLE,
           amd.EXPR_SQUARE, amd.EXPR_SCALE, amd.EXPR_HORNER, amd.EXPR_EMIT]
    assert ops == [E.COLUMN, E.CONST, E.ADD, E.SUB, E.MUL, E.NEG, E.DOUBLE, E.SQUARE, E.SCALE, E.HORNER, E.EMIT]
    assert ops == list(range(11)) and ctypes.sizeof(amd.ExprOp) == 12


@pytest.mark.parametrize("name", sorted(T.VALID))
def test_check_counts_equal_the_models(built, name):
    amd = A._amd()
    prog, ncol, ncon, nout = T.VALID[name]
    assert amd.expr_check(prog, ncol, ncon, nout) == E.check(prog, ncol, ncon, nout)


def test_check_table_has_the_lengths_and_depths_asked_for():
    depths = {name: E.check(*T.VALID[name])["depth"] for name in T.VALID}
    assert depths["depth_1"] == 1 and depths["depth_8"] == 8 and len(T.VALID["length_4096"][0]) == 4096
    assert len(T.MALFORMED["n_ops_0"][0]) == 0 and len(T.MALFORMED["n_ops_4097"][0]) == 4097


@pytest.mark.parametrize("name", sorted(T.MALFORMED))
def test_check_refuses_what_the_model_refuses(built, name):
    amd = A._amd()
    prog, ncol, ncon, nout = T.MALFORMED[name]
    with pytest.raises(E.ProgramError):
        E.check(prog, ncol, ncon, nout)
    with pytest.raises(amd.IcicleError) as e:
        amd.expr_check(prog, ncol, ncon, nout)
    assert e.value.code == amd.INVALID_ARGUMENT


def test_check_null_pointers(built):
    amd = A._amd()
    L = amd.lib()
    ops = amd._expr_program([(E.COLUMN, 0, 0), (E.EMIT, 0, 0)])
    out = (ctypes.c_int32 * 4)()
    assert L.mbls_fr_expr_check(None, 2, 1, 0, 1, out) == amd.INVALID_POINTER
    assert L.mbls_fr_expr_check(ops, 2, 1, 0, 1, None) == amd.INVALID_POINTER
    assert L.mbls_fr_expr_check(ops, 2, 1, 0, 1, out) == amd.SUCCESS and list(out) == [1, 1, 0, 1]


def test_eval_program_refuses_before_any_device_work(built):
    """every refusal of mbls_fr_eval_program comes before the first HIP call, so it answers here too"""
    amd = A._amd()
    L = amd.lib()
    col = (ctypes.c_uint64 * 8)()
    table = (ctypes.c_void_p * 2)(ctypes.addressof(col), ctypes.addressof(col))
    holed = (ctypes.c_void_p * 2)(ctypes.addressof(col), None)
    full = (ctypes.c_void_p * 1025)(*[ctypes.addressof(col)] * 1025)
    full[1023] = None
    ok = amd._expr_program([(E.COLUMN, 1, 0), (E.EMIT, 0, 0)])
    deep = amd._expr_program(T.MALFORMED["depth_9"][0])
    cfg = ctypes.byref(amd.vec_config())
    out = (ctypes.c_uint64 * 8)()
    P, A_ = amd.INVALID_POINTER, amd.INVALID_ARGUMENT
    cases = [
        (L.mbls_fr_eval_program(None, 2, 2, 1, None, 0, ok, 2, 1, cfg, out), P),
        (L.mbls_fr_eval_program(table, 2, 2, 1, None, 0, None, 2, 1, cfg, out), P),
        (L.mbls_fr_eval_program(table, 2, 2, 1, None, 0, ok, 2, 1, None, out), P),
        (L.mbls_fr_eval_program(table, 2, 2, 1, None, 0, ok, 2, 1, cfg, None), P),
        (L.mbls_fr_eval_program(table, 2, 2, 1, None, 1, ok, 2, 1, cfg, out), P),
        (L.mbls_fr_eval_program(holed, 2, 2, 1, None, 0, ok, 2, 1, cfg, out), P),
        (L.mbls_fr_eval_program(table, 2, 0, 1, None, 0, ok, 2, 1, cfg, out), A_),
        (L.mbls_fr_eval_program(table, 2, (1 << 26) + 1, 1, None, 0, ok, 2, 1, cfg, out), A_),
        (L.mbls_fr_eval_program(table, 2, 2, 0, None, 0, ok, 2, 1, cfg, out), A_),
        (L.mbls_fr_eval_program(table, 2, 2, (1 << 26) + 1, None, 0, ok, 2, 1, cfg, out), A_),
        (L.mbls_fr_eval_program(table, 1, 2, 1, None, 0, ok, 2, 1, cfg, out), A_),  # column 1 of 1
        (L.mbls_fr_eval_program(table, 2, 2, 1, None, 0, deep, 18, 1, cfg, out), A_),
        # a table of the most columns whose last is null: alone, then with a malformed program, no
        # rows, one column too many -- the program, the size and the count are looked at first
        (L.mbls_fr_eval_program(full, 1024, 2, 1, None, 0, ok, 2, 1, cfg, out), P),
        (L.mbls_fr_eval_program(full, 1024, 2, 1, None, 0, deep, 18, 1, cfg, out), A_),
        (L.mbls_fr_eval_program(full, 1024, 0, 1, None, 0, ok, 2, 1, cfg, out), A_),
        (L.mbls_fr_eval_program(full, 1025, 2, 1, None, 0, ok, 2, 1, cfg, out), A_),
    ]
    for k, (got, want) in enumerate(cases):
        assert got == want, k
    assert not any(out)
