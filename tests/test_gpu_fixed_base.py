"""Fixed-base batch multiplication (mbls_g*_fixed_base_table / _mul) and the SRS from a secret
(mbls_g1_srs_from_secret) on the GPU.

The oracle is the pure-Python restatement (oracle/pyref.py g1_mul / g2_mul): every element of every
batch is compared with the Montgomery affine limbs of the pyref result, bit for bit (the output is
canonical affine).  The expected points of the edge batches are computed once per module and shared
by the tests that slice them.  The digit width c and the window count W come from the plan, never
from a literal.  Two device-against-device tests need no oracle: the variable-base scalar_mul on a
replicated base, and the inverse EC-NTT of the monomial SRS, must give the same bytes."""
import ctypes
import random

import numpy as np
import pytest

import fixed_base_model as M
import helpers as H
from helpers import pyref as pr

pytestmark = pytest.mark.gpu

WORDS = {"g1": 12, "g2": 24}


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gpu_helpers
    gpu_helpers.amd.lib()
    return gpu_helpers.amd


def _enc(group, pts):
    enc = H.g1_affine_mont if group == "g1" else H.g2_affine_mont
    return np.array([enc(p) for p in pts], dtype=np.uint64).reshape(len(pts), WORDS[group])


def _scalars(vals):
    return H.ints_to_limbs([int(v) for v in vals], 4)


def _mont(vals):
    return _scalars([pr.fr_to_mont(int(v) % pr.R) for v in vals])


def _thin(sc, c):
    """the edge list thinned for G2: the fixed edges, the per-window cases of every fourth window and
    of the top two, the carry chains and the top-digit cases, 24 of the random values (more than 65
    scalars at every width, for the size cases)"""
    W = M.windows(c)
    keep = [w for w in range(W) if w % 4 == 0 or w >= W - 2]
    per_window = [sc[7 + 4 * w + j] for w in keep for j in range(4)]
    tail = sc[7 + 4 * W:]
    return sc[:7] + per_window + tail[:len(tail) - 64] + tail[-24:]


class Case:
    """one base, its device table and an edge batch with its expected affine rows"""

    def __init__(self, amd, group, seed):
        mul, gen = (pr.g1_mul, pr.G1) if group == "g1" else (pr.g2_mul, pr.G2)
        self.group, self.mul = group, mul
        self.plan = amd.fixed_base_plan(group)
        self.base = mul(random.Random(seed).randrange(1, pr.R), gen)
        self.base_limbs = _enc(group, [self.base])
        self.table = amd.fixed_base_table(group, self.base_limbs)
        sc = M.edge_scalars(self.plan["c"])
        if group == "g2":
            sc = _thin(sc, self.plan["c"])
        random.Random(seed + 1).shuffle(sc)  # every size below takes a mixed prefix
        self.sc = sc
        self.want = _enc(group, [mul(s % pr.R, self.base) for s in sc])


@pytest.fixture(scope="module")
def g1(amd):
    return Case(amd, "g1", 0xFB01)


@pytest.fixture(scope="module")
def g2(amd):
    return Case(amd, "g2", 0xFB02)


def _same(got, want, sc, what):
    assert got.shape == want.shape
    for i in range(len(want)):
        assert got[i].tobytes() == want[i].tobytes(), (what, i, hex(sc[i]))


def test_edge_batch_sizes(g1, g2):
    c, W = g1.plan["c"], g1.plan["W"]
    assert 7 + 4 * W + 64 <= len(g1.sc) < 300 and 65 <= len(g2.sc) <= 130 and len(g1.sc) >= 129
    for case in (g1, g2):
        s = set(case.sc)
        assert {0, 1, 2, pr.R - 1, pr.R, pr.R + 1, (1 << 256) - 1} <= s
        # the digit -2^(c-1) with its carry into the top window, and the top window's lowest bit
        assert (1 << (c - 1)) << (c * (W - 2)) in s and 1 << (c * (W - 1)) in s
        # the largest top digit: that of r - 1 (the top digit does not decrease with k)
        assert max(M.recode(k, c)[-1] for k in s) == M.recode(pr.R - 1, c)[-1]
        assert sum(1 for k, w in zip(case.sc, case.want) if not w.any()) >= 2  # 0 and r


@pytest.mark.parametrize("mont", [False, True])
def test_g1_edge_scalars(amd, g1, mont):
    sc = _mont(g1.sc) if mont else _scalars(g1.sc)
    _same(amd.fixed_base_mul("g1", g1.table, sc, scalars_mont=mont), g1.want, g1.sc, ("g1", mont))


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_g1_sizes(amd, g1, n, mont):
    sc = _mont(g1.sc[:n]) if mont else _scalars(g1.sc[:n])
    _same(amd.fixed_base_mul("g1", g1.table, sc, scalars_mont=mont), g1.want[:n], g1.sc, ("g1", n, mont))


@pytest.mark.parametrize("mont", [False, True])
def test_g2_edge_scalars(amd, g2, mont):
    sc = _mont(g2.sc) if mont else _scalars(g2.sc)
    _same(amd.fixed_base_mul("g2", g2.table, sc, scalars_mont=mont), g2.want, g2.sc, ("g2", mont))


@pytest.mark.parametrize("n", [1, 64, 65])
def test_g2_sizes(amd, g2, n):
    _same(amd.fixed_base_mul("g2", g2.table, _scalars(g2.sc[:n])), g2.want[:n], g2.sc, ("g2", n))


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_identity_base(amd, g1, g2, group):
    case = g1 if group == "g1" else g2
    table = amd.fixed_base_table(group, np.zeros((1, WORDS[group]), dtype=np.uint64))
    assert not amd.to_numpy_u64(table).any()
    out = np.full((len(case.sc), WORDS[group]), 0xA5, dtype=np.uint64)
    amd.fixed_base_mul(group, table, _scalars(case.sc), out=out)
    assert not out.any()


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_table_contents(amd, g1, g2, group):
    case = g1 if group == "g1" else g2
    c, W, rows = case.plan["c"], case.plan["W"], case.plan["rows"]
    tab = amd.to_numpy_u64(case.table)
    assert tab.shape == (case.plan["entries"], WORDS[group]) and rows == 1 << (c - 1)
    for w in (0, 1, W - 1):
        for d in (1, 2, rows - 1, rows):
            idx = M.table_index(w, d, c)
            assert idx == w * rows + d - 1 and M.table_scalar(idx, c) == d << (c * w)
            want = _enc(group, [case.mul((d << (c * w)) % pr.R, case.base)])
            assert tab[idx].tobytes() == want[0].tobytes(), (group, w, d)
    assert tab.any(axis=1).all()


def test_placement_combinations(amd, g1):
    """host / device base, scalars and output give the same bytes"""
    n = 65
    sc = _scalars(g1.sc[:n])
    dev_table = amd.fixed_base_table("g1", amd.torch_u64(g1.base_limbs))
    assert np.array_equal(amd.to_numpy_u64(dev_table), amd.to_numpy_u64(g1.table))
    for sd in (False, True):
        for od in (False, True):
            out = amd.torch_u64((n, 12)) if od else None
            got = amd.fixed_base_mul("g1", dev_table, amd.torch_u64(sc) if sd else sc, out=out)
            got = amd.to_numpy_u64(got) if od else got
            _same(got, g1.want[:n], g1.sc, (sd, od))


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_async_on_a_side_stream(amd, g1, g2, group):
    import torch
    case = g1 if group == "g1" else g2
    n = 65
    s = amd.torch_u64(_scalars(case.sc[:n]))
    out = amd.torch_u64((n, WORDS[group]))
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())  # after the fills of s and out
    table = amd.fixed_base_table(group, case.base_limbs, stream=st, is_async=True)
    amd.fixed_base_mul(group, table, s, out=out, stream=st, is_async=True)
    st.synchronize()
    _same(amd.to_numpy_u64(out), case.want[:n], case.sc, (group, "async"))
    assert torch.equal(table, case.table)
    amd.release_stream(st)


def test_no_allocation_after_warm_up(amd, g1):
    sc = _scalars(g1.sc[:65])
    tau = _mont([7])[0]
    # two warm-up rounds: these calls hold one scratch context and the entries they run lease a
    # second, and which of the pool's contexts plays which part settles after the first round
    for _ in range(2):
        first = amd.fixed_base_mul("g1", g1.table, sc), amd.srs_from_secret(g1.table, tau, 64, lagrange=True)
        amd.fixed_base_table("g1", g1.base_limbs)
    m0, f0 = amd.scratch_stats()[:2]
    second = amd.fixed_base_mul("g1", g1.table, sc), amd.srs_from_secret(g1.table, tau, 64, lagrange=True)
    amd.fixed_base_table("g1", g1.base_limbs)
    m1, f1 = amd.scratch_stats()[:2]
    assert (m1, f1) == (m0, f0)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_against_variable_base_scalar_mul(amd, g1, g2, group):
    """device against device: a batch past the per-launch lane limit plus 77, scalars from
    mbls_gen_scalars; mbls_g*_scalar_mul on a replicated base followed by projective_to_affine gives
    the same bytes"""
    import torch
    case = g1 if group == "g1" else g2
    chunk = case.plan["chunk"]
    n = (chunk if chunk else 1 << 12) + 77
    nl = WORDS[group]
    s = amd.torch_u64((n, 4))
    amd.gen_scalars(s, 0xF1BA5E02, montgomery=False)
    got = amd.torch_u64((n, nl))
    amd.fixed_base_mul(group, case.table, s, out=got)
    bases = amd.torch_u64(case.base_limbs).repeat(n, 1).contiguous()
    jac = amd.torch_u64((n, nl * 3 // 2))
    amd.scalar_mul(group, bases, s, out=jac)
    want = amd.torch_u64((n, nl))
    amd.convert_points(group, "to_affine", jac, out=want)
    torch.cuda.synchronize()
    assert bool(want.any(dim=1).all())
    assert torch.equal(got, want)
    # the Montgomery form of the same scalars
    sm = amd.torch_u64((n, 4))
    amd.gen_scalars(sm, 0xF1BA5E02, montgomery=True)
    got2 = amd.torch_u64((n, nl))
    amd.fixed_base_mul(group, case.table, sm, scalars_mont=True, out=got2)
    assert torch.equal(got2, want)


# ----------------------------------------------------------------------------- SRS
def _lagrange_at(tau, n):
    """L_i(tau) over the Fr NTT's domain of size n, from the definition prod_(j != i) (tau - w^j) /
    (w^i - w^j) -- not the barycentric formula the library uses"""
    w = pr.omega(n.bit_length() - 1)
    xs = [pow(w, i, pr.R) for i in range(n)]
    out = []
    for i in range(n):
        num = den = 1
        for j in range(n):
            if j != i:
                num = num * (tau - xs[j]) % pr.R
                den = den * (xs[i] - xs[j]) % pr.R
        out.append(num * pow(den, -1, pr.R) % pr.R)
    return out


def _tau(v):
    return _mont([v])[0]


def test_srs_monomial_against_pyref(amd, g1):
    n = 16
    tau = random.Random(0xFB10).randrange(2, pr.R)
    got = amd.srs_from_secret(g1.table, _tau(tau), n)
    ks = [pow(tau, i, pr.R) for i in range(n)]
    _same(got, _enc("g1", [pr.g1_mul(k, g1.base) for k in ks]), ks, "monomial")
    # any size, not only a power of two
    assert np.array_equal(amd.srs_from_secret(g1.table, _tau(tau), 13), got[:13])


@pytest.mark.parametrize("n", [8, 64])
def test_srs_lagrange_against_pyref(amd, g1, n):
    tau = random.Random(0xFB20 + n).randrange(2, pr.R)
    ks = _lagrange_at(tau, n)
    assert sum(ks) % pr.R == 1
    got = amd.srs_from_secret(g1.table, _tau(tau), n, lagrange=True)
    _same(got, _enc("g1", [pr.g1_mul(k, g1.base) for k in ks]), ks, ("lagrange", n))


@pytest.mark.parametrize("n", [1, 64, 256])
def test_srs_lagrange_equals_inverse_ecntt_of_monomial(amd, g1, n):
    """the two routes share no group code past the table"""
    import torch
    tau = _tau(random.Random(0xFB30 + n).randrange(2, pr.R))
    mono, lag = amd.torch_u64((n, 12)), amd.torch_u64((n, 12))
    amd.srs_from_secret(g1.table, tau, n, out=mono)
    amd.srs_from_secret(g1.table, tau, n, lagrange=True, out=lag)
    via = amd.torch_u64((n, 12))
    amd.ecntt(mono, inverse=True, out=via)
    assert bool(lag.any(dim=1).all())
    assert torch.equal(lag, via)
    assert np.array_equal(amd.srs_from_secret(g1.table, tau, n, lagrange=True), amd.to_numpy_u64(lag))  # host output


def test_srs_refuses_a_root_of_unity(amd, g1):
    out = np.zeros((16, 12), dtype=np.uint64)
    w3 = _tau(pow(pr.omega(3), 3, pr.R))
    cfg = amd.vec_config(is_a_on_device=True)
    call = amd.lib().mbls_g1_srs_from_secret
    assert call(amd._p(g1.table), amd._p(w3), 8, 1, ctypes.byref(cfg), amd._p(out)) == amd.INVALID_ARGUMENT
    assert call(amd._p(g1.table), amd._p(w3), 16, 1, ctypes.byref(cfg), amd._p(out)) == amd.INVALID_ARGUMENT
    assert not out.any()
    assert call(amd._p(g1.table), amd._p(w3), 4, 1, ctypes.byref(cfg), amd._p(out)) == amd.SUCCESS  # w^3 has order 8
    # the monomial basis has no pole
    assert call(amd._p(g1.table), amd._p(w3), 8, 0, ctypes.byref(cfg), amd._p(out)) == amd.SUCCESS


def test_srs_domain_order_bounds_the_lagrange_size(amd, g1):
    out = np.zeros((16, 12), dtype=np.uint64)
    cfg = amd.vec_config(is_a_on_device=True)
    call = amd.lib().mbls_g1_srs_from_secret
    tau = _tau(5)
    try:
        w8 = pr.int_to_limbs(pr.fr_to_mont(pr.omega(3)), 4)
        amd.ntt_init_domain(np.array(w8, dtype=np.uint64))
        assert call(amd._p(g1.table), amd._p(tau), 8, 1, ctypes.byref(cfg), amd._p(out)) == amd.SUCCESS
        assert call(amd._p(g1.table), amd._p(tau), 16, 1, ctypes.byref(cfg), amd._p(out)) == amd.INVALID_ARGUMENT
        assert call(amd._p(g1.table), amd._p(tau), 16, 0, ctypes.byref(cfg), amd._p(out)) == amd.SUCCESS
    finally:
        amd.ntt_init_domain()


def test_srs_of_tau_zero(amd, g1):
    """tau = 0: the monomial SRS is [base, 0, 0, ..] (0^0 = 1).  The Lagrange SRS of the same
    polynomial basis is NOT that vector: L_i(0) = (0 - 1)/n * w^i / (0 - w^i) = 1/n for every i (the
    L_i sum to one), which is also what the inverse EC-NTT of [base, 0, 0, ..] gives."""
    n = 8
    zero = _tau(0)
    mono = amd.srs_from_secret(g1.table, zero, n)
    assert np.array_equal(mono[:1], g1.base_limbs) and not mono[1:].any()
    lag = amd.srs_from_secret(g1.table, zero, n, lagrange=True)
    want = _enc("g1", [pr.g1_mul(pow(n, -1, pr.R), g1.base)])
    assert np.array_equal(lag, np.repeat(want, n, axis=0))
    assert np.array_equal(lag, amd.ecntt(mono, inverse=True))


# ----------------------------------------------------------------------------- nested leases
# The table build, the G2 multiplication and the SRS call hold a scratch context and run other
# entries of the library, which lease a second one.  A thread that holds a context must never wait
# for another: the calls below would otherwise stop for good once every context is held by a caller
# that waits for a second.
def _nested_digest(amd, stream=None):
    """every entry that nests a lease, once, on the generators; the SHA-256 of all outputs"""
    import hashlib
    import torch
    kw = dict(stream=stream, is_async=stream is not None)
    n = 64
    sc = amd.torch_u64(_scalars([(0x9E3779B97F4A7C15 * (i + 1)) ** 3 % pr.R for i in range(n)]))
    t1 = amd.fixed_base_table("g1", _enc("g1", [pr.G1]), **kw)
    t2 = amd.fixed_base_table("g2", _enc("g2", [pr.G2]), **kw)
    # empty, not zeros: a fill on torch's current stream could land after the writes on `stream`
    o2, lag, mono = (torch.empty((n, w), dtype=torch.int64, device="cuda") for w in (24, 12, 12))
    amd.fixed_base_mul("g2", t2, sc, out=o2, **kw)
    amd.srs_from_secret(t1, _tau(0xC0FFEE), n, lagrange=True, out=lag, **kw)
    amd.srs_from_secret(t1, _tau(0xC0FFEE), n, out=mono, **kw)
    (stream.synchronize if stream is not None else torch.cuda.synchronize)()
    h = hashlib.sha256()
    for t in (t1, t2, o2, lag, mono):
        h.update(amd.to_numpy_u64(t).tobytes())
    return h.hexdigest()


def test_more_threads_than_scratch_contexts(amd):
    """8 threads, twice the pool's default limit of 4, each on a stream of its own, run the nesting
    entries at the same moment, four rounds each: every call returns and gives the single-threaded
    bytes"""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    import torch
    want = _nested_digest(amd)
    threads = 8
    streams = [torch.cuda.Stream() for _ in range(threads)]
    gate = threading.Barrier(threads)

    def work(k):
        torch.cuda.set_device(0)
        gate.wait(60)
        return [_nested_digest(amd, streams[k]) for _ in range(4)]

    with ThreadPoolExecutor(threads) as ex:
        futures = [ex.submit(work, k) for k in range(threads)]
        got = [f.result(timeout=300) for f in futures]
    assert all(d == want for ds in got for d in ds)
    for st in streams:
        amd.release_stream(st)
    assert amd.scratch_stats()[3] <= 4 + threads  # at most one context past the limit per nested thread


def test_one_scratch_context_is_enough():
    """MBLS_SCRATCH_CONTEXTS=1 (read once per process, hence a child): the nested lease gets a
    context past the limit instead of waiting on its own caller"""
    import os
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import torch; import gpu_helpers; import test_gpu_fixed_base as T; "
            "a = gpu_helpers.amd; print('digest', T._nested_digest(a), a.scratch_stats()[3])" % os.path.dirname(__file__))
    outs = []
    for limit in ("1", "4"):
        env = dict(os.environ, MBLS_SCRATCH_CONTEXTS=limit)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([l for l in r.stdout.splitlines() if l.startswith("digest")][0].split())
    assert outs[0][1] == outs[1][1]
    assert int(outs[0][2]) == 2 and int(outs[1][2]) <= 4
