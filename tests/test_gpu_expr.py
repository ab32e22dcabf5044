"""The Fr expression evaluator (mbls_fr_eval_program) on the GPU against the pure-Python interpreter
of tests/expr_model.py.  Every comparison is exact equality of the element words.  Sizes are the
seams of the 256-row tile and of the rotation wrap, not workload sizes.  The operand pool is computed
once: every column is a window of it."""
import ctypes
import functools
import random

import numpy as np
import pytest

import expr_model as E
import scan_model as M

pytestmark = pytest.mark.gpu

TILE = 256
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2 * TILE + 3)
POOL = 1031  # a prime: no tile repeats its neighbour's operands


def _amd():
    """the binding, with torch imported before the library is loaded: a process that loads the
    library first and torch afterwards ends with a HIP runtime that reports no device"""
    import torch  # noqa: F401
    import gpu_helpers
    return gpu_helpers.amd


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _amd().lib()
    return _amd()


def words(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def ints(arr):
    data = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def dev(a):
    return _amd().torch_u64(np.ascontiguousarray(a))


def host(t):
    return _amd().to_numpy_u64(t)


@functools.lru_cache(maxsize=None)
def pool():
    """0, 1, r - 1 and random values, Montgomery form, cycled with a prime period"""
    rnd = random.Random(41)
    return tuple(E.mont(rnd.choice([0, 1, E.R - 1] + [rnd.randrange(E.R) for _ in range(5)])) for _ in range(POOL))


def column(n, start):
    """n operands from the pool, from `start` on"""
    p = pool()
    return [p[(start + i) % POOL] for i in range(n)]


CONSTS = [E.mont(v) for v in (0, 1, E.R - 1, 0x1234567890abcdef1234567890abcdef, E.R - 2, 7)]


def run_both(amd, cols, prog, consts=(), n_outputs=1, rot_stride=1, on_device=True):
    """(the library's outputs, the model's), both as lists of int lists"""
    n = len(cols[0])
    place = dev if on_device else (lambda a: a)
    got = amd.eval_program([place(words(c)) for c in cols], prog, constants=place(words(consts)) if consts else None,
                           n_outputs=n_outputs, rot_stride=rot_stride)
    got = ints(host(got) if on_device else got)
    return [got[k * n:(k + 1) * n] for k in range(n_outputs)], E.run(cols, prog, consts, n_outputs, rot_stride)


X0 = (E.EMIT, 0, 0)
ALONE = {
    "column": [(E.COLUMN, 1, 0), X0],
    "const": [(E.CONST, 3, 0), X0],
    "add": [(E.COLUMN, 0, 0), (E.COLUMN, 1, 0), (E.ADD, 0, 0), X0],
    "sub": [(E.COLUMN, 0, 0), (E.COLUMN, 1, 0), (E.SUB, 0, 0), X0],
    "mul": [(E.COLUMN, 0, 0), (E.COLUMN, 1, 0), (E.MUL, 0, 0), X0],
    "neg": [(E.COLUMN, 0, 0), (E.NEG, 0, 0), X0],
    "double": [(E.COLUMN, 0, 0), (E.DOUBLE, 0, 0), X0],
    "square": [(E.COLUMN, 0, 0), (E.SQUARE, 0, 0), X0],
    "scale": [(E.COLUMN, 0, 0), (E.SCALE, 3, 0), X0],
    "scale_by_minus_one": [(E.COLUMN, 0, 0), (E.SCALE, 2, 0), X0],
    "horner": [(E.COLUMN, 0, 0), (E.COLUMN, 1, 0), (E.HORNER, 4, 0), X0],
    "emit_two": [(E.COLUMN, 0, 0), (E.COLUMN, 1, 0), (E.EMIT, 1, 0), X0],
}


@pytest.mark.parametrize("name", sorted(ALONE))
def test_every_opcode_alone(amd, name):
    n_out = 2 if name == "emit_two" else 1
    for n in SIZES:
        # two windows 257 apart: every pair of 0, 1, r - 1 and random operands meets somewhere
        cols = [column(n, 0), column(n, 257)]
        got, want = run_both(amd, cols, ALONE[name], CONSTS, n_out)
        assert got == want, n
        assert all(v < E.R for o in got for v in o), n


@pytest.mark.parametrize("size", [257, 1000])
@pytest.mark.parametrize("stride", [1, 4])
def test_rotations_read_the_right_row(amd, size, stride):
    """element i encodes i: a wrong row shows as a wrong index.  257 puts the wrap inside a tile,
    1000 lets a rotated tile straddle two workgroups' rows."""
    col = [E.mont(i) for i in range(size)]
    for b in (-(size - 1), -1, 0, 1, size - 1, size + 5, -3 * size - 2):
        got, want = run_both(amd, [col], [(E.COLUMN, 0, b), X0], rot_stride=stride)
        assert got == want, b
        assert got[0] == [E.mont((i + b * stride) % size) for i in range(size)], b
    # several rotations of one column in one program
    prog = [(E.COLUMN, 0, -1), (E.COLUMN, 0, 1), (E.SUB, 0, 0), (E.COLUMN, 0, size + 5), (E.ADD, 0, 0), X0]
    got, want = run_both(amd, [col], prog, rot_stride=stride)
    assert got == want


def sub_chain(depth):
    """`depth` columns pushed, then depth - 1 SUBs: c0 - (c1 - (c2 - ...)), every slot distinct"""
    return [(E.COLUMN, k, 0) for k in range(depth)] + [(E.SUB, 0, 0)] * (depth - 1) + [X0]


def test_stack_depths(amd):
    n = 257
    cols = [column(n, 37 * k + 3) for k in range(8)]
    full = None
    for depth in (8, 7, 2):
        prog = sub_chain(depth)
        assert E.check(prog, 8, 0, 1)["depth"] == depth
        got, want = run_both(amd, cols, prog)
        assert got == want, depth
        full = full or got
    # SUB is not commutative: the chain over the reversed columns is another column
    assert run_both(amd, cols[::-1], sub_chain(8))[0] != full
    # interleaved push / pop: slots are left and taken again at several depths
    prog = [(E.COLUMN, 0, 0), (E.COLUMN, 1, 0), (E.COLUMN, 2, 0), (E.SUB, 0, 0), (E.COLUMN, 3, 1), (E.COLUMN, 4, -1),
            (E.COLUMN, 5, 0), (E.MUL, 0, 0), (E.SUB, 0, 0), (E.SUB, 0, 0), (E.COLUMN, 6, 2), (E.EMIT, 1, 0),
            (E.COLUMN, 7, 0), (E.COLUMN, 0, 3), (E.SUB, 0, 0), (E.SUB, 0, 0), (E.SUB, 0, 0), X0]
    got, want = run_both(amd, cols, prog, n_outputs=2)
    assert got == want


def perm_inputs(m, n):
    cols = [column(n, 53 * k + 1) for k in range(2 * m)] + [[E.mont(pow(7, i, E.R)) for i in range(n)]]
    beta, gamma, delta = 0xbe7a, 0x9a33a, 11
    return cols, [E.mont(beta * pow(delta, k, E.R)) for k in range(m)] + [E.mont(beta), E.mont(gamma)]


def test_permutation_feeds_the_grand_product(amd):
    m, n = 3, 1024
    cols, consts = perm_inputs(m, n)
    got, want = run_both(amd, cols, E.permutation(m), consts, n_outputs=2)
    assert got == want
    # on the device, straight into the scan: z[i] = prod_{j < i} num[j] / den[j]
    out = amd.eval_program([dev(words(c)) for c in cols], E.permutation(m), constants=dev(words(consts)), n_outputs=2)
    z = amd.prefix_product(out[:n], out[n:], out=amd.torch_u64((n, 4)))
    assert ints(host(z)) == M.prefix_product_ref(want[0], want[1])[0]


def test_eight_outputs_in_reverse_order(amd):
    n = 65
    cols = [column(n, 11 * k) for k in range(8)]
    prog = []
    for k in range(7, -1, -1):  # output k = column k, doubled k times
        prog += [(E.COLUMN, k, 0)] + [(E.DOUBLE, 0, 0)] * k + [(E.EMIT, k, 0)]
    got, want = run_both(amd, cols, prog, n_outputs=8)
    assert got == want
    assert got[0] == cols[0] and got[1] == [2 * v % E.R for v in cols[1]]


def test_long_random_program(amd):
    n = 65
    prog = E.random_program(4, 4096, 8, 16, 16)
    assert len(prog) == 4096 and E.check(prog, 16, 16, 1)["depth"] == 8
    cols = [column(n, 61 * k + 5) for k in range(16)]
    consts = column(16, 700)
    got, want = run_both(amd, cols, prog, consts)
    assert got == want


def test_horner_and_scale_equal_const_mul_add(amd):
    n = 2 * TILE + 3
    cols = [column(n, 101 * k + 9) for k in range(4)]
    y = [CONSTS[3]]
    fused, want = run_both(amd, cols, E.gate_fold(True), y)
    plain, want2 = run_both(amd, cols, E.gate_fold(False), y)
    assert fused == want and plain == want2 and fused == plain


def test_placement_and_stream(amd):
    import torch
    m, n = 3, 2 * TILE + 3
    cols, consts = perm_inputs(m, n)
    prog = E.permutation(m)
    d_out, want = run_both(amd, cols, prog, consts, n_outputs=2)
    h_out, _ = run_both(amd, cols, prog, consts, n_outputs=2, on_device=False)
    assert d_out == want and h_out == want
    # device columns, host constants, host output; and the reverse
    mixed = amd.eval_program([dev(words(c)) for c in cols], prog, constants=words(consts), n_outputs=2,
                             out=np.zeros((2 * n, 4), dtype=np.uint64))
    assert ints(mixed) == want[0] + want[1]
    mixed = amd.eval_program([words(c) for c in cols], prog, constants=dev(words(consts)), n_outputs=2,
                             out=amd.torch_u64((2 * n, 4)))
    assert ints(host(mixed)) == want[0] + want[1]
    # asynchronous on a stream of its own
    st = torch.cuda.Stream()
    dcols, dconsts, out = [dev(words(c)) for c in cols], dev(words(consts)), amd.torch_u64((2 * n, 4))
    torch.cuda.synchronize()
    amd.eval_program(dcols, prog, constants=dconsts, n_outputs=2, out=out, stream=st, is_async=True)
    st.synchronize()
    assert ints(host(out)) == want[0] + want[1]
    amd.release_stream(st)


def test_errors_leave_the_output_untouched(amd):
    L, P = amd.lib(), amd._p
    n = 257
    col = dev(words(column(n, 0)))
    fill = np.full((n, 4), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    out = dev(fill)
    cfg = amd.vec_config(is_a_on_device=True, is_b_on_device=True, is_result_on_device=True)
    ok = amd._expr_program([(E.COLUMN, 1, 0), X0])
    holed = (ctypes.c_void_p * 2)(col.data_ptr(), None)
    assert L.mbls_fr_eval_program(holed, 2, n, 1, None, 0, ok, 2, 1, ctypes.byref(cfg), P(out)) == amd.INVALID_POINTER
    deep = [(E.COLUMN, 0, 0)] * 9 + [(E.ADD, 0, 0)] * 8 + [X0]
    with pytest.raises(amd.IcicleError) as e:
        amd.eval_program([col], deep, out=out)
    assert e.value.code == amd.INVALID_ARGUMENT
    assert np.array_equal(host(out), fill)
    # the same buffers with a well-formed call do get written
    amd.eval_program([col, col], [(E.COLUMN, 1, 0), X0], out=out)
    assert np.array_equal(host(out), host(col))


def test_no_allocation_on_a_second_call(amd):
    m, n = 3, 2 * TILE + 3
    cols, consts = perm_inputs(m, n)
    dcols, dconsts, out = [dev(words(c)) for c in cols], dev(words(consts)), amd.torch_u64((2 * n, 4))
    hcols, hconsts = [words(c) for c in cols], words(consts)

    def calls():
        amd.eval_program(dcols, E.permutation(m), constants=dconsts, n_outputs=2, out=out)
        amd.eval_program(hcols, E.permutation(m), constants=hconsts, n_outputs=2)  # staged: the largest footprint

    calls()
    mallocs = amd.scratch_stats()[0]
    calls()
    assert amd.scratch_stats()[0] == mallocs
