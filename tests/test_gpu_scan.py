"""The Fr scans (mbls_fr_prefix_product, mbls_fr_poly_divide_linear) on the GPU against the
pure-Python recurrences of tests/scan_model.py.  Every comparison is exact equality of the element
words.  Sizes come from mbls_fr_scan_geometry, not from literals: chunk, tile and span seams, and
both sides of the size at which a workgroup first gets a second tile.  One reference column of that
size is computed once; every smaller size is a slice of it (a prefix for the products, a suffix for
the division)."""
import ctypes
import functools
import random

import numpy as np
import pytest

import scan_model as M

pytestmark = pytest.mark.gpu


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
def geometry():
    """(K, T, n2): elements per thread and per tile, and the first size whose spans hold two tiles"""
    geo = _amd().scan_geometry
    K, T = geo(1)["K"], geo(1)["tile"]
    lo, hi = 1, 1 << 26  # span(lo) == T < span(hi)
    assert geo(lo)["span"] == T < geo(hi)["span"]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if geo(mid)["span"] > T else (mid, hi)
    assert geo(hi)["groups"] < geo(lo)["groups"]  # the workgroup count stopped growing at lo
    return K, T, hi


def seam_sizes():
    K, T, n2 = geometry()
    return sorted({1, 2, K - 1, K, K + 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, n2 - 1, n2, n2 + 1} - {0})


RND = random.Random(2024)
INIT = M.mont(RND.randrange(1, M.R))
Z = M.mont(RND.randrange(2, M.R - 1))
POINTS = {"zero": 0, "one": M.ONE, "minus_one": M.mont(M.R - 1), "random": Z}


@functools.lru_cache(maxsize=None)
def big():
    """The shared reference.  col: n2 + 1 values without a zero, a pool of 4099 (a prime: no tile or
    span repeats a neighbour's values) of 1, r - 1 and random ones, cycled.  prefix[i] = INIT *
    prod_{j < i} col[j]; suffix[i] = col[i] + Z * suffix[i + 1], suffix[n] = 0.  All as word arrays."""
    n = geometry()[2] + 1
    rnd = random.Random(11)
    pool = [M.mont(rnd.choice([1, M.R - 1] + [rnd.randrange(1, M.R) for _ in range(6)])) for _ in range(4099)]
    pw = words(pool)
    col = np.ascontiguousarray(np.tile(pw, (n // 4099 + 1, 1))[:n])
    rinv = M.pr.FR_RINV
    fac = [v * rinv % M.R for v in pool]  # a Montgomery product is a plain product by x / R
    prefix, run = [], INIT
    for i in range(n):
        prefix.append(run)
        run = run * fac[i % 4099] % M.R
    prefix.append(run)
    zc = Z * rinv % M.R
    suffix, run = [0] * (n + 1), 0
    for i in range(n - 1, -1, -1):
        run = (pool[i % 4099] + zc * run) % M.R
        suffix[i] = run
    return col, words(prefix), words(suffix)


def test_reference_slices_match_the_model():
    """the shared reference, sliced as the tests slice it, is the model's recurrence"""
    col, prefix, suffix = big()
    n = len(col)
    c = ints(col[:100])
    out, total = M.prefix_product_ref(c, init=INIT)
    assert out == ints(prefix[:100]) and total == ints(prefix[100:101])[0]
    q, ev = M.divide_ref(ints(col[n - 100:]), Z)
    assert q == ints(suffix[n - 99:]) and ev == ints(suffix[n - 100:n - 99])[0]


@pytest.mark.parametrize("inclusive", [False, True])
def test_prefix_product_at_every_seam(amd, inclusive):
    col, prefix, _ = big()
    init = words([INIT])
    for n in seam_sizes():
        out, total = amd.prefix_product(col[:n], init=init, inclusive=inclusive, total=True)
        want = prefix[1:n + 1] if inclusive else prefix[:n]
        assert np.array_equal(out, want), n
        assert np.array_equal(total, prefix[n:n + 1]), n


def test_poly_divide_linear_at_every_seam(amd):
    col, _, suffix = big()
    N = len(col)
    z = words([Z])
    for n in seam_sizes():
        q, ev = amd.poly_divide_linear(col[N - n:], z)
        assert np.array_equal(q, suffix[N - n + 1:]), n
        assert np.array_equal(ev, suffix[N - n:N - n + 1]), n


def _edge_column(n, seed):
    rnd = random.Random(seed)
    return [M.mont(rnd.choice([0, 1, M.R - 1] + [rnd.randrange(M.R) for _ in range(5)])) for _ in range(n)]


@pytest.mark.parametrize("point", sorted(POINTS))
def test_division_edge_values(amd, point):
    K, T, _ = geometry()
    z = POINTS[point]
    for n in (K + 1, 2 * T + 3):
        a = _edge_column(n, n)
        q, ev = amd.poly_divide_linear(words(a), words([z]))
        wq, wev = M.divide_ref(a, z)
        assert ints(q) == wq and ints(ev) == [wev], n
        if point == "zero":  # the coefficients shifted down by one
            assert ints(q) == a[1:] + [0] and ints(ev) == [a[0]]
        if point == "one":  # the suffix sums (Montgomery form is linear)
            sums = [sum(a[i + 1:]) % M.R for i in range(n)] if n < 100 else None
            assert sums is None or ints(q) == sums
            assert ints(ev) == [sum(a) % M.R]


def test_zero_at_a_chunk_tile_and_span_seam(amd):
    """a zero at the last element of a chunk, the first of a tile inside a span and the first of a
    span: everything after it is 0, and nothing before it is touched"""
    K, T, n2 = geometry()
    col, prefix, _ = big()
    n = n2 + 1
    span = amd.scan_geometry(n)["span"]
    assert span == 2 * T
    zero = np.zeros((1, 4), dtype=np.uint64)
    for pos in (K - 1, T, span, 3 * span + T):
        x = col[:n].copy()
        x[pos] = 0
        out, total = amd.prefix_product(x, init=words([INIT]), total=True)
        assert np.array_equal(out[:pos + 1], prefix[:pos + 1]), pos
        assert not out[pos + 1:].any() and not total.any(), pos
        assert out[:pos + 1].any(axis=1).all(), pos
        inc = amd.prefix_product(x, init=words([INIT]), inclusive=True)
        assert np.array_equal(inc[:pos], prefix[1:pos + 1]) and not inc[pos:].any(), pos
    # small sizes, one workgroup: the same three places exist at 2 T + 3 (spans of one tile)
    m = 2 * T + 3
    for pos in (K - 1, T - 1, T, 2 * T):
        x = col[:m].copy()
        x[pos] = 0
        out = amd.prefix_product(x, init=words([INIT]))
        assert np.array_equal(out[:pos + 1], prefix[:pos + 1]) and not out[pos + 1:].any(), pos


def test_denominators(amd):
    K, T, _ = geometry()
    n = 2 * T + 3
    rnd = random.Random(3)
    num = [M.mont(rnd.randrange(1, M.R)) for _ in range(n)]
    den = [M.mont(rnd.randrange(1, M.R)) for _ in range(n)]
    ones = words([M.ONE] * n)
    # den == NULL is den of all ones
    plain, tp = amd.prefix_product(words(num), init=words([INIT]), total=True)
    out, total = amd.prefix_product(words(num), ones, init=words([INIT]), total=True)
    assert np.array_equal(out, plain) and np.array_equal(total, tp)
    # zero denominators at the seams, from the last one to the first: 1 / 0 = 0
    for pos in (None, 2 * T, T, T - 1, K - 1):
        if pos is not None:
            den[pos] = 0
        for inclusive in (False, True):
            out, total = amd.prefix_product(words(num), words(den), init=words([INIT]), inclusive=inclusive, total=True)
            wout, wtotal = M.prefix_product_ref(num, den, INIT, inclusive)
            assert ints(out) == wout and ints(total) == [wtotal], (pos, inclusive)
    # a zero numerator and a zero denominator elsewhere: the earlier one decides
    num[K + 1] = 0
    out = amd.prefix_product(words(num), words(den))
    assert ints(out) == M.prefix_product_ref(num, den)[0]


def test_init_and_total_chain_across_calls(amd):
    """a column split at an arbitrary point into two calls, the first's device total the second's
    init, equals one call over the whole column; no init is Montgomery one"""
    K, T, _ = geometry()
    col, _, _ = big()
    n, cut = 3 * T + 5, T + K + 3
    x = dev(col[:n])
    whole, wt = amd.prefix_product(x, out=amd.torch_u64((n, 4)), total=True)
    out = amd.torch_u64((n, 4))
    _, t1 = amd.prefix_product(x[:cut], out=out[:cut], total=True, is_async=True)
    _, t2 = amd.prefix_product(x[cut:], init=t1, out=out[cut:], total=True)
    assert np.array_equal(host(out), host(whole)) and np.array_equal(host(t2), host(wt))
    one = amd.prefix_product(col[:n], init=words([M.ONE]))
    assert np.array_equal(one, host(whole))
    assert ints(one[:3]) == M.prefix_product_ref(ints(col[:3]))[0]


def test_batch_members_equal_single_calls(amd):
    K, T, _ = geometry()
    col, _, _ = big()
    n, b = T + 1, 3
    x = col[:b * n]
    rnd = random.Random(9)
    per = words([M.mont(rnd.randrange(1, M.R)) for _ in range(b)])
    out, total = amd.prefix_product(x, init=per, batch=b, total=True)
    inc = amd.prefix_product(x, x[::-1].copy(), init=per, batch=b, inclusive=True)
    q, ev = amd.poly_divide_linear(x, per, batch=b)
    for k in range(b):
        xs, s = x[k * n:(k + 1) * n], slice(k * n, (k + 1) * n)
        o1, t1 = amd.prefix_product(xs, init=per[k:k + 1], total=True)
        assert np.array_equal(out[s], o1) and np.array_equal(total[k:k + 1], t1), k
        i1 = amd.prefix_product(xs, x[::-1][s].copy(), init=per[k:k + 1], inclusive=True)
        assert np.array_equal(inc[s], i1), k
        q1, e1 = amd.poly_divide_linear(xs, per[k:k + 1])
        assert np.array_equal(q[s], q1) and np.array_equal(ev[k:k + 1], e1), k
    # the members differ, so a member that read its neighbour's z or init would show
    assert len({tuple(r) for r in total.tolist()}) == b and len({tuple(r) for r in ev.tolist()}) == b
    with pytest.raises(amd.IcicleError) as e:
        cfg = amd.vec_config(batch_size=b, columns_batch=True)
        amd.check(amd.lib().mbls_fr_prefix_product(amd._p(x), None, n, None, False, ctypes.byref(cfg), amd._p(out), None),
                  "prefix_product")
    assert e.value.code == amd.API_NOT_IMPLEMENTED
    with pytest.raises(amd.IcicleError) as e:
        amd.check(amd.lib().mbls_fr_poly_divide_linear(amd._p(x), n, amd._p(per), ctypes.byref(cfg), amd._p(q), None),
                  "poly_divide_linear")
    assert e.value.code == amd.API_NOT_IMPLEMENTED


def test_placement_and_in_place(amd):
    K, T, _ = geometry()
    col, prefix, suffix = big()
    n, N = T + 1, len(col)
    num, den, a = col[:n], col[n:2 * n], col[N - n:]
    init, z = words([INIT]), words([Z])
    # all-host operands equal all-device operands
    h_out, h_tot = amd.prefix_product(num, den, init=init, total=True)
    d_out, d_tot = amd.prefix_product(dev(num), dev(den), init=dev(init), out=amd.torch_u64((n, 4)), total=True)
    assert np.array_equal(h_out, host(d_out)) and np.array_equal(h_tot, host(d_tot))
    hq, hev = amd.poly_divide_linear(a, z)
    dq, dev_ev = amd.poly_divide_linear(dev(a), dev(z), out=amd.torch_u64((n, 4)))
    assert np.array_equal(hq, suffix[N - n + 1:]) and np.array_equal(hev, suffix[N - n:N - n + 1])
    assert np.array_equal(host(dq), hq) and np.array_equal(host(dev_ev), hev)
    # in place: output is num, output is den, quotient is coeffs
    t = dev(num)
    assert amd.prefix_product(t, dev(den), init=init, out=t) is t and np.array_equal(host(t), h_out)
    t = dev(den)
    amd.prefix_product(dev(num), t, init=init, out=t)
    assert np.array_equal(host(t), h_out)
    t = dev(num)
    amd.prefix_product(t, init=init, out=t)
    assert np.array_equal(host(t), prefix[:n])
    t = dev(a)
    amd.poly_divide_linear(t, z, out=t)
    assert np.array_equal(host(t), hq)
    # either output alone
    none, ev = amd.poly_divide_linear(a, z, quotient=False)
    assert none is None and np.array_equal(ev, hev)
    q, none = amd.poly_divide_linear(a, z, eval=False)
    assert none is None and np.array_equal(q, hq)
    ev = amd.poly_divide_linear(dev(a), dev(z), quotient=False, eval=amd.torch_u64((1, 4)))[1]
    assert np.array_equal(host(ev), hev)


def test_one_large_size_checked_on_the_device(amd):
    """n = 2^22 + 1, verified with the element-wise vecops on shifted views, no Python loop"""
    import torch
    n = (1 << 22) + 1
    x = amd.torch_u64((n, 4))
    amd.gen_scalars(x, 77, montgomery=True)
    init, z = words([INIT]), words([Z])
    out, total = amd.prefix_product(x, init=init, out=amd.torch_u64((n, 4)), total=True)
    step = amd.vec_op("mul", out, x, out=amd.torch_u64((n, 4)))  # step[i] = out[i] * x[i] = out[i + 1]
    assert torch.equal(step[:-1], out[1:]) and torch.equal(step[-1:], total)
    assert np.array_equal(host(out[:1]), init) and total.any()
    q, ev = amd.poly_divide_linear(x, z, out=amd.torch_u64((n, 4)))
    zq = amd.vec_op("scalar_mul", z, q, out=amd.torch_u64((n, 4)))
    back = amd.vec_op("sub", q[:-1], zq[1:], out=amd.torch_u64((n - 1, 4)))  # q[i-1] - z q[i] = a[i]
    assert torch.equal(back, x[1:])
    a0 = amd.vec_op("sub", ev, zq[:1], out=amd.torch_u64((1, 4)))  # p(z) - z q[0] = a[0]
    assert torch.equal(a0, x[:1]) and not host(q[-1:]).any()


def test_errors_come_before_any_device_work(amd):
    L, P = amd.lib(), amd._p
    buf = np.zeros((8, 4), dtype=np.uint64)
    one = np.zeros((1, 4), dtype=np.uint64)
    cfg = amd.vec_config()
    two = amd.vec_config(batch_size=2)
    c, c2 = ctypes.byref(cfg), ctypes.byref(two)
    amd.prefix_product(buf)  # a first call, so that the scratch pool exists
    before = amd.scratch_stats()
    big_n = (1 << 26) + 1
    cases = [
        (L.mbls_fr_prefix_product(None, None, 8, None, False, c, P(buf), None), amd.INVALID_POINTER),
        (L.mbls_fr_prefix_product(P(buf), None, 8, None, False, None, P(buf), None), amd.INVALID_POINTER),
        (L.mbls_fr_prefix_product(P(buf), None, 8, None, False, c, None, P(one)), amd.INVALID_POINTER),
        (L.mbls_fr_prefix_product(P(buf), None, 0, None, False, c, P(buf), None), amd.INVALID_ARGUMENT),
        (L.mbls_fr_prefix_product(P(buf), None, big_n, None, False, c, P(buf), None), amd.INVALID_ARGUMENT),
        (L.mbls_fr_prefix_product(P(buf), None, (1 << 25) + 1, None, False, c2, P(buf), None), amd.INVALID_ARGUMENT),
        (L.mbls_fr_poly_divide_linear(None, 8, P(one), c, P(buf), P(one)), amd.INVALID_POINTER),
        (L.mbls_fr_poly_divide_linear(P(buf), 8, None, c, P(buf), P(one)), amd.INVALID_POINTER),
        (L.mbls_fr_poly_divide_linear(P(buf), 8, P(one), None, P(buf), P(one)), amd.INVALID_POINTER),
        (L.mbls_fr_poly_divide_linear(P(buf), 8, P(one), c, None, None), amd.INVALID_POINTER),
        (L.mbls_fr_poly_divide_linear(P(buf), 0, P(one), c, P(buf), P(one)), amd.INVALID_ARGUMENT),
        (L.mbls_fr_poly_divide_linear(P(buf), big_n, P(one), c, P(buf), P(one)), amd.INVALID_ARGUMENT),
        (L.mbls_fr_poly_divide_linear(P(buf), (1 << 25) + 1, P(buf), c2, P(buf), P(one)), amd.INVALID_ARGUMENT),
    ]
    for k, (got, want) in enumerate(cases):
        assert got == want, k
    assert amd.scratch_stats() == before


def test_no_allocation_per_call(amd):
    K, T, _ = geometry()
    col, _, _ = big()
    n = 2 * T + 3
    x, d, z = dev(col[:n]), dev(col[n:2 * n]), dev(words([Z]))
    out, tot = amd.torch_u64((n, 4)), amd.torch_u64((1, 4))

    def calls():
        amd.prefix_product(x, d, out=out, total=tot)
        amd.prefix_product(col[:n], col[n:2 * n], total=True)  # staged: the largest footprint
        amd.poly_divide_linear(x, z, out=out, eval=tot)

    calls()
    mallocs = amd.scratch_stats()[0]
    for _ in range(10):
        calls()
    assert amd.scratch_stats()[0] == mallocs
