"""The Fr inner products (mbls_fr_inner_products, mbls_fr_multi_eval, mbls_fr_powers) on the GPU
against the pure-Python sums of tests/inner_model.py and against the library's own scans, NTT and
vector operations.  Every comparison is exact equality of the element words.  Sizes come from
mbls_fr_inner_plan, not from literals: the tile seams, the block seams CB and VB, and one size above
which a workgroup takes several tiles.  One bank of columns is made once; every case slices it."""
import functools
import random

import numpy as np
import pytest

import inner_model as M

pytestmark = pytest.mark.gpu

R = M.R


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
def plan():
    p = _amd().inner_plan(1)
    return p["tile"], p["CB"], p["VB"]


def seam_sizes():
    T = plan()[0]
    return [1, 2, T - 1, T, T + 1, 3 * T + 5]


BANK_ROWS = 19  # 3 columns + 16 vectors at the most


@functools.lru_cache(maxsize=None)
def bank():
    """BANK_ROWS distinct columns of 3T + 5 values: 0, 1, r - 1 and random ones from a pool of 4099 (a
    prime: no tile repeats a neighbour's values), each column starting elsewhere in the pool.
    Returns (integer lists, word arrays)."""
    n = 3 * plan()[0] + 5
    rnd = random.Random(515)
    pool = [M.mont(rnd.choice([0, 1, R - 1] + [rnd.randrange(R) for _ in range(9)])) for _ in range(4099)]
    cols = [[pool[(i + 211 * k) * (k + 1) % 4099] for i in range(n)] for k in range(BANK_ROWS)]
    return cols, [words(c) for c in cols]


def case(nc, nv, n):
    """nc columns and nv vectors of n rows: (column ints, vector ints, column words, vector words)"""
    ci, cw = bank()
    assert nc + nv <= BANK_ROWS + 1
    cols, vecs = list(range(nc)), list(range(BANK_ROWS - nv, BANK_ROWS))
    return ([ci[k][:n] for k in cols], [ci[k][:n] for k in vecs],
            [np.ascontiguousarray(cw[k][:n]) for k in cols], [np.ascontiguousarray(cw[k][:n]) for k in vecs])


RND = random.Random(99)
Z = M.mont(RND.randrange(2, R - 1))
POINTS = [0, M.ONE, M.mont(R - 1), Z]


def test_inner_products_at_every_seam(amd):
    for n in seam_sizes():
        ci, vi, cw, vw = case(3, 2, n)
        got = amd.inner_products(cw, vw)
        assert got.shape == (6, 4) and ints(got) == M.inner_products_ref(ci, vi), n


def test_a_workgroup_with_several_tiles(amd):
    """one column by one vector just above the size at which the row groups stop growing; the
    expected value is the library's own product and sum"""
    import torch
    T = plan()[0]
    n = amd.inner_plan(1)["group_cap"] * T + T + 1
    assert amd.inner_plan(n)["tiles_per_group"] == 2 and amd.inner_plan(n - T - 1)["tiles_per_group"] == 1
    a, b = amd.torch_u64((n, 4)), amd.torch_u64((n, 4))
    amd.gen_scalars(a, 71, montgomery=True)
    amd.gen_scalars(b, 72, montgomery=True)
    prod = amd.torch_u64((n, 4))
    amd.vec_op("mul", a, b, out=prod)
    want = amd.vector_sum(prod)
    got = amd.inner_products([a], [b])
    torch.cuda.synchronize()
    assert np.array_equal(host(got), want) and want.any()


@pytest.mark.parametrize("nv", ["1", "VB", "VB+1", "16"])
def test_block_seams(amd, nv):
    T, CB, VB = plan()
    nv = {"1": 1, "VB": VB, "VB+1": VB + 1, "16": 16}[nv]
    for nc in sorted({1, CB, CB + 1}):
        ci, vi, cw, vw = case(nc, nv, T + 1)
        want = M.inner_products_ref(ci, vi)
        assert len(set(want)) == nc * nv  # distinct outputs: a swapped index shows
        assert ints(amd.inner_products(cw, vw)) == want, (nc, nv)


def test_extremes_every_word_pattern_r_minus_one(amd):
    """7 maximal canonical products in every deferred accumulator of the full tiles"""
    T, CB, VB = plan()
    n = 3 * T + 5
    top = words([R - 1] * n)
    nc, nv = CB + 1, VB + 1
    stats = {}
    g = M.Geometry(2, amd.inner_plan(1)["defer"], CB, VB, 1)
    small = M.blocked_inner([[R - 1] * 40], [[R - 1] * 40], g, stats)  # the model's bound assertions run
    assert stats["most"] == M.DEFER == g.defer and small == M.inner_products_ref([[R - 1] * 40], [[R - 1] * 40])
    want = [n * (R - 1) * (R - 1) * M.RINV % R] * (nc * nv)
    assert want == M.inner_products_ref([[R - 1] * n], [[R - 1] * n]) * (nc * nv)
    assert ints(amd.inner_products([top] * nc, [top] * nv)) == want


def test_multi_eval_equals_the_eval_only_scan(amd):
    n = 3 * plan()[0] + 5
    ci, _, cw, _ = case(3, 1, n)
    pts = words(POINTS)
    got = amd.multi_eval([dev(c) for c in cw], dev(pts), out=amd.torch_u64((3 * len(POINTS), 4)))
    for p in range(3):
        for k in range(len(POINTS)):
            _, ev = amd.poly_divide_linear(dev(cw[p]), dev(pts[k:k + 1]), quotient=False, eval=amd.torch_u64((1, 4)))
            assert np.array_equal(host(ev)[0], host(got)[p * len(POINTS) + k]), (p, k)
    assert ints(host(got)) == M.multi_eval_ref(ci, POINTS)
    assert ints(host(got)[0:1]) == [ci[0][0]]  # z = 0 gives a[0]


def test_multi_eval_at_roots_of_unity_is_the_ntt(amd):
    log_n = 11
    n = 1 << log_n
    _, _, cw, _ = case(1, 1, n)
    amd.ntt_init_domain()
    evals = amd.ntt(cw[0])
    w = M.pr.omega(log_n)
    js = [0, 1, 2, 5, n // 2, n - 1]
    pts = words([M.mont(pow(w, j, R)) for j in js])
    got = amd.multi_eval(cw, pts)
    for k, j in enumerate(js):
        assert np.array_equal(got[k], evals[j]), j


def test_powers(amd):
    base3 = [Z, M.mont(R - 1), M.mont(3)]
    init3 = [M.mont(RND.randrange(1, R)), M.mont(7), 0]
    for n in seam_sizes():
        got = amd.powers(words(base3), n, init=words(init3))
        want = [v for b, i in zip(base3, init3) for v in M.powers_ref(b, n, i)]
        assert ints(got) == want, n
        assert ints(amd.powers(words([Z]), n)) == M.powers_ref(Z, n), n  # init omitted
    assert ints(amd.powers(words([0, M.ONE]), 5, init=words([Z, Z]))) == [Z, 0, 0, 0, 0] + [Z] * 5
    assert ints(amd.powers(words([0]), 1)) == [M.ONE]


def test_powers_then_inner_products_is_multi_eval(amd):
    n = plan()[0] + 1
    _, _, cw, _ = case(3, 1, n)
    pts = words(POINTS)
    pw = amd.powers(dev(pts), n)
    vecs = [pw[k * n:(k + 1) * n] for k in range(len(POINTS))]
    cols = [dev(c) for c in cw]
    a, b = amd.inner_products(cols, vecs), amd.multi_eval(cols, dev(pts))
    assert np.array_equal(host(a), host(b)) and host(a).any()


def test_barycentric_evaluation_of_a_lagrange_column(amd):
    """sum_i f_i L_i(z), L_i(z) = (z^n - 1) / n * w^i / (z - w^i), from powers (init carrying the
    constant), scalar_add_vec, batch_inv, vector_mul and inner_products, against multi_eval of the
    column's inverse NTT"""
    log_n = 11
    n = 1 << log_n
    _, _, cw, _ = case(1, 1, n)
    amd.ntt_init_domain()
    coeffs = amd.ntt(cw[0], inverse=True)
    want = amd.multi_eval([coeffs], words([Z]))
    zs, w = M.pr.fr_from_mont(Z), M.pr.omega(log_n)
    c = (1 - pow(zs, n, R)) * pow(n, -1, R) % R  # L_i(z) = c * w^i / (w^i - z)
    wi = amd.powers(dev(words([M.mont(w)])), n)
    cwi = amd.powers(dev(words([M.mont(w)])), n, init=dev(words([M.mont(c)])))
    den = amd.torch_u64((n, 4))
    amd.vec_op("scalar_add", dev(words([M.mont(-zs)])), wi, out=den)
    amd.batch_inv(den, den)
    lag = amd.torch_u64((n, 4))
    amd.vec_op("mul", cwi, den, out=lag)
    got = amd.inner_products([dev(cw[0])], [lag])
    assert np.array_equal(host(got), want) and want.any()


def test_placement(amd):
    import torch
    n = plan()[0] + 1
    ci, vi, cw, vw = case(3, 2, n)
    want = words(M.inner_products_ref(ci, vi))
    cd, vd = [dev(c) for c in cw], [dev(v) for v in vw]
    assert np.array_equal(amd.inner_products(cw, vw), want)  # all host
    assert np.array_equal(host(amd.inner_products(cd, vd)), want)  # all device
    assert np.array_equal(amd.inner_products(cd, vw, out=np.zeros((6, 4), dtype=np.uint64)), want)
    assert np.array_equal(host(amd.inner_products(cw, vd, out=amd.torch_u64((6, 4)))), want)
    pts = words(POINTS)
    wev = words(M.multi_eval_ref(ci, POINTS))
    assert np.array_equal(amd.multi_eval(cw, pts), wev)
    assert np.array_equal(host(amd.multi_eval(cd, dev(pts))), wev)
    assert np.array_equal(host(amd.multi_eval(cw, dev(pts), out=amd.torch_u64((12, 4)))), wev)
    assert np.array_equal(amd.multi_eval(cd, pts, out=np.zeros((12, 4), dtype=np.uint64)), wev)
    wpw = words(M.powers_ref(Z, n))
    assert np.array_equal(amd.powers(words([Z]), n), wpw)
    assert np.array_equal(host(amd.powers(dev(words([Z])), n)), wpw)
    assert np.array_equal(host(amd.powers(words([Z]), n, out=amd.torch_u64((n, 4)))), wpw)
    # a non-default stream, asynchronous: the results are there once the stream is synchronised
    s = torch.cuda.Stream()
    o1, o2, o3 = amd.torch_u64((6, 4)), amd.torch_u64((12, 4)), amd.torch_u64((n, 4))
    dp, dz = dev(pts), dev(words([Z]))
    torch.cuda.synchronize()
    amd.inner_products(cd, vd, out=o1, stream=s, is_async=True)
    amd.multi_eval(cd, dp, out=o2, stream=s, is_async=True)
    amd.powers(dz, n, out=o3, stream=s, is_async=True)
    s.synchronize()
    assert np.array_equal(host(o1), want) and np.array_equal(host(o2), wev) and np.array_equal(host(o3), wpw)


def test_no_allocation_per_call(amd):
    n = 3 * plan()[0] + 5
    _, _, cw, vw = case(3, 2, n)
    cd, vd, pts = [dev(c) for c in cw], [dev(v) for v in vw], words(POINTS)
    o1, o2, o3 = amd.torch_u64((6, 4)), amd.torch_u64((12, 4)), amd.torch_u64((2 * n, 4))

    def calls():
        amd.inner_products(cd, vd, out=o1)
        amd.inner_products(cw, vw)  # staged: the largest footprint
        amd.multi_eval(cw, pts)
        amd.multi_eval(cd, dev(pts), out=o2)
        amd.powers(words([Z, Z]), n, out=o3)

    calls()
    mallocs = amd.scratch_stats()[0]
    for _ in range(10):
        calls()
    assert amd.scratch_stats()[0] == mallocs
