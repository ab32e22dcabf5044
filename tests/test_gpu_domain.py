"""The extended-coset transforms on the device (mbls_fr_coeff_to_extended, mbls_fr_extended_to_coeff)
against tests/domain_model.py, against the model's closed forms, and, byte for byte, against the
composed path of the same build (zero-pad + bls12_381_coset_ntt_cuda, which the parity tests pin to
the oracle).  Every output word is compared.

Sizes: one size per pass-plan shape -- one pass (log2 N in 0, 1, 2, 3, 6, 8), two passes (9 with
L = 5, 4; 10; 12), three passes (17, the smallest).  At each, E runs over 0..log2 N, so it crosses
E = L and E = L + 1 of the first pass (where the pruning is capped) and size = 1."""
import functools

import numpy as np
import pytest

import domain_model as D
import ntt_model as NM
from helpers import pyref as pr

R = pr.R
gpu = pytest.mark.gpu
SMALL = [0, 1, 2, 3, 6, 8, 9, 10, 12]
GENS = list(D.GENERATORS)


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gpu_helpers
    gpu_helpers.amd.lib()
    gpu_helpers.amd.ntt_init_domain()
    return gpu_helpers.amd


def _rand(seed, n):
    g = pr.rng(seed)
    return [g.randrange(R) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _rand_limbs(seed, n):
    v = _rand(seed, n)
    return v, D.to_mont_limbs(v)


def _gw(name):
    return None if name is None else D.mont_words(D.GENERATORS[name])


def _sizes(K, E):
    base = 1 << (K - E)
    return sorted({s for s in (base, base - 1, base + 1, 3) if 1 <= s <= 1 << K})


@pytest.fixture(scope="module")
def plain_before(amd):
    """the plain and the coset NTT at 2^9, before this module's first domain call"""
    _, x = _rand_limbs(0xB4, 1 << 9)
    return (amd.ntt(x.copy()), amd.ntt(x.copy(), inverse=True),
            amd.ntt(x.copy(), coset_gen=_gw("zeta"), entry="coset"),
            amd.ntt(x.copy(), inverse=True, coset_gen=_gw("zeta"), entry="coset"))


# ----------------------------------------------------------------------------- forward
@gpu
@pytest.mark.parametrize("K", SMALL)
def test_forward_vs_model(amd, plain_before, K):
    N = 1 << K
    vals, limbs = _rand_limbs(0xF0 + K, N)
    k = 0
    for E in range(K + 1):
        for size in _sizes(K, E):
            # every generator at E = 0, 2, K and around the first pass's L; one in rotation elsewhere
            L0 = D.plan(size, N)["plan"][0][1] if K else 0
            names = GENS if E in (0, 2, L0, L0 + 1, K) and size == 1 << (K - E) else [GENS[k % len(GENS)]]
            k += 1
            for name in names:
                got = amd.coeff_to_extended(limbs[:size].copy(), N, _gw(name))
                want = D.to_mont_limbs(D.coeff_to_extended(vals[:size], N, D.GENERATORS[name]))
                assert np.array_equal(got, want), (K, E, size, name)
            if names is GENS:  # NULL is Montgomery one
                assert np.array_equal(amd.coeff_to_extended(limbs[:size].copy(), N, None),
                                      amd.coeff_to_extended(limbs[:size].copy(), N, _gw("one")))


def _composed_forward(amd, limbs, N, g):
    import torch
    pad = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    pad[:limbs.shape[0]] = amd.torch_u64(limbs)
    out = torch.zeros_like(pad)
    amd.ntt(pad, out=out, coset_gen=g, entry="coset")
    return amd.to_numpy_u64(out)


@gpu
@pytest.mark.parametrize("E", [0, 2, 3, 7])
def test_forward_2_17(amd, plain_before, E):
    K = 17
    N, size = 1 << K, 1 << (K - E)
    assert len(D.plan(size, N)["plan"]) == 3
    _, limbs = _rand_limbs(0x17, N)
    for s in (size, size - 1, (size >> 1) + 1):  # the last two: partly filled rows, same E
        for name in ("zeta", "rand", "one"):
            got = amd.coeff_to_extended(limbs[:s].copy(), N, _gw(name))
            assert np.array_equal(got, _composed_forward(amd, limbs[:s], N, _gw(name))), (E, s, name)
    g = D.ZETA
    for v in (1, R - 1, D.FIXED_RANDOM):
        for q in (0, size - 1):
            a = np.zeros((q + 1, 4), dtype=np.uint64)
            a[q] = D.mont_words(v)
            got = amd.coeff_to_extended(a, N, D.mont_words(g))
            assert np.array_equal(got, D.to_mont_limbs(D.monomial_extended(v, q, N, g))), (E, v, q)
    for c, gg in ((1, D.ZETA), (R - 1, R - 1), (D.FIXED_RANDOM, 7)):
        a = np.tile(np.array(D.mont_words(c), dtype=np.uint64), (size, 1))
        got = amd.coeff_to_extended(a, N, D.mont_words(gg))
        assert np.array_equal(got, D.to_mont_limbs(D.constant_run_extended(c, size, N, gg))), (E, c)


# ----------------------------------------------------------------------------- inverse
def _out_sizes(K, E):
    N = 1 << K
    return sorted({m for m in (1, 1 << (K - E), 3 * (N >> 2), N - 1, N) if 1 <= m <= N})


def _periods(K, E):
    return [None] + sorted({1, 1 << E, 1 << K})


@gpu
@pytest.mark.parametrize("K", SMALL)
def test_inverse_vs_model(amd, plain_before, K):
    N = 1 << K
    vals, limbs = _rand_limbs(0x1F0 + K, N)
    vv, vl = _rand_limbs(0x2F0 + K, N)
    k = 0
    for E in sorted({0, min(2, K), K}):
        for period in _periods(K, E):
            name = GENS[k % len(GENS)]
            k += 1
            vinv = None if period is None else vv[:period]
            full = D.extended_to_coeff(vals, N, N, D.GENERATORS[name], vinv)
            for m in _out_sizes(K, E):
                got = amd.extended_to_coeff(limbs.copy(), m, _gw(name), None if period is None else vl[:period].copy())
                assert got.shape == (m, 4)
                assert np.array_equal(got, D.to_mont_limbs(full[:m])), (K, E, period, m, name)
    # every generator, no vanishing division; NULL is Montgomery one
    for name in GENS:
        want = D.to_mont_limbs(D.extended_to_coeff(vals, N, N, D.GENERATORS[name]))
        assert np.array_equal(amd.extended_to_coeff(limbs.copy(), N, _gw(name)), want), (K, name)
    assert np.array_equal(amd.extended_to_coeff(limbs.copy(), N, None), amd.extended_to_coeff(limbs.copy(), N, _gw("one")))


@gpu
@pytest.mark.parametrize("E", [0, 2, 3, 7])
def test_inverse_2_17_vs_composed(amd, plain_before, E):
    import torch
    K = 17
    N = 1 << K
    _, limbs = _rand_limbs(0x117, N)
    _, vl = _rand_limbs(0x217, N)
    e = amd.torch_u64(limbs)
    for period, name in zip(_periods(K, E), ("zeta", "rand", "zeta", "one")):
        if period is None:
            ev, vdev = e, None
        else:
            vdev = amd.torch_u64(vl[:period].copy())
            ev = torch.zeros_like(e)
            amd.vec_op("mul", e, vdev.repeat(N // period, 1), out=ev)
        want = torch.zeros_like(e)
        amd.ntt(ev, inverse=True, out=want, coset_gen=_gw(name), entry="coset")
        want = amd.to_numpy_u64(want)
        for m in _out_sizes(K, E):
            out = torch.full((m + 1, 4), -1, dtype=torch.int64, device="cuda")  # one guard row
            amd.extended_to_coeff(e, m, _gw(name), vdev, out=out)
            got = amd.to_numpy_u64(out)
            assert np.array_equal(got[:m], want[:m]), (E, period, m, name)
            assert (got[m] == np.uint64(2 ** 64 - 1)).all(), "wrote past out_size"
    assert np.array_equal(amd.to_numpy_u64(e), limbs), "the input was written"


# ----------------------------------------------------------------------------- reduction boundaries
def _boundary_inputs(N):
    return {"all_r-1": [R - 1] * N, "zeros": [0] * N, "alternating": [0 if i % 2 == 0 else R - 1 for i in range(N)],
            # the Montgomery WORD r - 1 in every element
            "word_r-1": [pr.fr_from_mont(R - 1)] * N}


@gpu
@pytest.mark.parametrize("K", [3, 9, 12])
def test_reduction_boundaries(amd, plain_before, K):
    N = 1 << K
    vinv = [R - 1] * 4
    for nm, x in _boundary_inputs(N).items():
        xl = D.to_mont_limbs(x)
        for name in ("r-1", "zeta", "one"):
            g = D.GENERATORS[name]
            for E in (0, 2):
                size = N >> E
                got = amd.coeff_to_extended(xl[:size].copy(), N, _gw(name))
                assert np.array_equal(got, D.to_mont_limbs(D.coeff_to_extended(x[:size], N, g))), (nm, name, E, "fwd")
            for v, vl in ((None, None), (vinv, D.to_mont_limbs(vinv))):
                got = amd.extended_to_coeff(xl.copy(), N, _gw(name), vl)
                assert np.array_equal(got, D.to_mont_limbs(D.extended_to_coeff(x, N, N, g, v))), (nm, name, "inv")


# ----------------------------------------------------------------------------- the prover's shape
@gpu
def test_halo2_shape_and_round_trip(amd, plain_before):
    k, j = 10, 4
    dom = D.Halo2Domain(k, j)
    assert (dom.extended_k, len(dom.t_evaluations)) == (12, 4)
    m = 3 << k
    a, al = _rand_limbs(0xA2, dom.n)
    zeta = D.mont_words(D.ZETA)
    ext = amd.coeff_to_extended(al.copy(), dom.N, zeta)
    assert np.array_equal(ext, D.to_mont_limbs(dom.coeff_to_extended(a)))
    assert np.array_equal(amd.extended_to_coeff(ext, dom.n, zeta), al)  # the round trip
    h, hl = _rand_limbs(0xA3, dom.N)
    want = dom.extended_to_coeff(dom.divide_by_vanishing_poly(h))
    assert len(want) == m
    got = amd.extended_to_coeff(hl.copy(), m, zeta, D.to_mont_limbs(dom.t_evaluations))
    assert np.array_equal(got, D.to_mont_limbs(want))


@gpu
def test_batch_of_three(amd, plain_before):
    N, size, m = 1 << 9, 1 << 7, 3 << 7
    vals, limbs = _rand_limbs(0xB3, 3 * N)
    g = D.mont_words(D.ZETA)
    for s in (size, size - 1):
        x = np.concatenate([limbs[b * N:b * N + s] for b in range(3)])
        got = amd.coeff_to_extended(x, N, g, batch=3)
        want = np.concatenate([D.to_mont_limbs(D.coeff_to_extended(vals[b * N:b * N + s], N, D.ZETA)) for b in range(3)])
        assert np.array_equal(got, want), s
    vv, vl = _rand_limbs(0xB5, 4)
    got = amd.extended_to_coeff(limbs.copy(), m, g, vl.copy(), batch=3)
    want = np.concatenate([D.to_mont_limbs(D.extended_to_coeff(vals[b * N:(b + 1) * N], N, m, D.ZETA, vv)) for b in range(3)])
    assert np.array_equal(got, want)


@gpu
@pytest.mark.parametrize("in_dev", [False, True])
@pytest.mark.parametrize("out_dev", [False, True])
def test_placement(amd, plain_before, in_dev, out_dev):
    import torch
    N, size, m = 1 << 10, 1 << 8, 3 << 8
    vals, limbs = _rand_limbs(0xC1, N)
    vv, vl = _rand_limbs(0xC2, 4)
    g = D.mont_words(7)
    put = (lambda a: amd.torch_u64(a.copy())) if in_dev else (lambda a: a.copy())
    mk = (lambda n: torch.zeros((n, 4), dtype=torch.int64, device="cuda")) if out_dev else \
        (lambda n: np.zeros((n, 4), dtype=np.uint64))
    back = amd.to_numpy_u64 if out_dev else (lambda a: a)
    out = mk(N)
    amd.coeff_to_extended(put(limbs[:size]), N, g, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(back(out), D.to_mont_limbs(D.coeff_to_extended(vals[:size], N, 7)))
    out = mk(m)
    amd.extended_to_coeff(put(limbs), m, g, put(vl), out=out)
    torch.cuda.synchronize()
    assert np.array_equal(back(out), D.to_mont_limbs(D.extended_to_coeff(vals, N, m, 7, vv)))


@gpu
def test_async_on_a_stream(amd, plain_before):
    import torch
    N, size, m = 1 << 12, 1 << 10, 3 << 10
    vals, limbs = _rand_limbs(0xD1, N)
    vv, vl = _rand_limbs(0xD2, 4)
    g = D.mont_words(D.ZETA)
    st = torch.cuda.Stream()
    x, e, v = amd.torch_u64(limbs[:size].copy()), amd.torch_u64(limbs), amd.torch_u64(vl)
    ext = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    co = torch.zeros((m, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        amd.coeff_to_extended(x, N, g, out=ext, stream=st, is_async=True)
        amd.extended_to_coeff(e, m, g, v, out=co, stream=st, is_async=True)
    st.synchronize()
    assert np.array_equal(amd.to_numpy_u64(ext), D.to_mont_limbs(D.coeff_to_extended(vals[:size], N, D.ZETA)))
    assert np.array_equal(amd.to_numpy_u64(co), D.to_mont_limbs(D.extended_to_coeff(vals, N, m, D.ZETA, vv)))


@gpu
def test_scratch_use(amd, plain_before):
    import torch
    N, size, m = 1 << 12, 1 << 10, 3 << 10
    _, limbs = _rand_limbs(0xE1, N)
    g = D.mont_words(D.ZETA)
    x, e, v = amd.torch_u64(limbs[:size].copy()), amd.torch_u64(limbs), amd.torch_u64(limbs[:4].copy())
    ext = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    co = torch.zeros((m, 4), dtype=torch.int64, device="cuda")

    def calls():
        amd.extended_to_coeff(e, m, g, v, out=co)
        amd.extended_to_coeff(limbs.copy(), m, g, limbs[:4].copy())  # staged: the largest footprint
        amd.coeff_to_extended(limbs[:size].copy(), N, g)

    calls()
    before = amd.scratch_stats()
    for _ in range(3):
        calls()
    assert amd.scratch_stats()[0] == before[0], "an allocation on a later call of the same shape"
    # device operands: the forward call works in its output and takes no scratch context
    before = amd.scratch_stats()
    amd.coeff_to_extended(x, N, g, out=ext)
    amd.coeff_to_extended(x, N, None, out=ext)
    torch.cuda.synchronize()
    assert amd.scratch_stats() == before
    assert amd.domain_plan(size, N)["fwd_scratch"] == 0 and amd.domain_plan(size, N)["inv_scratch"] == N


# ----------------------------------------------------------------------------- one engine, two kernels
@gpu
@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 12, 13, 17])
def test_full_size_unit_coset_equals_plain_ntt(amd, plain_before, K):
    """k_dom_pass and k_ntt_pass run one stage engine in different modes, so with nothing for the
    domain passes to add (size = N: no pruning; no generator; no vanishing table; out_size = N) they
    give the plain transforms' bytes.  The sizes are the plan shapes of test_gpu_ntt.py's
    test_pass_plans_of_the_gpu_sizes: the lone radix-2 stage, the trivial pair alone, pair + tail, the
    largest single pass, clamped logC, full tiles, an odd L in a first pass that is not the last (13,
    which no other test of this module runs), and the first plan with a middle pass."""
    N = 1 << K
    # canonical, seeded; the seeds are those of test_forward_2_17 and test_forward_vs_model, so that
    # _rand_limbs' cache hands back their arrays and 2^17 values are not drawn and converted twice
    _, x = _rand_limbs(0x17 if K == 17 else 0xF0 + K, N)
    assert np.array_equal(amd.coeff_to_extended(x.copy(), N, None), amd.ntt(x.copy())), K
    assert np.array_equal(amd.extended_to_coeff(x.copy(), N, None, None), amd.ntt(x.copy(), inverse=True)), K


# ----------------------------------------------------------------------------- the NTT entries, after
@gpu
def test_plain_ntt_unchanged_afterwards(amd, plain_before):
    """the last test of the module: after every domain call above, the plain and the coset NTT at
    2^9 still give their bytes from before"""
    vals, x = _rand_limbs(0xB4, 1 << 9)
    after = (amd.ntt(x.copy()), amd.ntt(x.copy(), inverse=True),
             amd.ntt(x.copy(), coset_gen=_gw("zeta"), entry="coset"),
             amd.ntt(x.copy(), inverse=True, coset_gen=_gw("zeta"), entry="coset"))
    for b, a in zip(plain_before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(after[0], D.to_mont_limbs(pr.ntt_forward(vals)))
