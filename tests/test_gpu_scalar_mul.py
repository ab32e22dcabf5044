"""Batch scalar multiplication (bls12_381_g1_scalar_mul, _glv, bls12_381_g2_scalar_mul and the
mbls_* forms) on the GPU against the pure-Python restatement (oracle/pyref.py g1_mul / g2_mul).

Every element of every batch is checked.  Values are compared as affine points: the raw Jacobian
output goes through the library's projective_to_affine and must equal the Montgomery affine
limbs of the pyref result bit for bit; where the expected point is the identity the raw output's
Z is also asserted zero.  The G1 kernel recodes each 128-bit GLV half into 32 signed 4-bit
digits; the G2 kernel walks the bits of four 63-bit psi digits."""
import ctypes
import random

import numpy as np
import pytest

import helpers as H
from helpers import pyref as pr

pytestmark = pytest.mark.gpu

WINDOW = 4   # G1 digit width (csrc/scalar_mul.hip)
BLOCK = 64   # lanes per workgroup (SM_BLOCK)
ENTRIES = ("bls12_381_g1_scalar_mul", "bls12_381_g1_scalar_mul_glv", "bls12_381_g2_scalar_mul",
           "mbls_g1_scalar_mul", "mbls_g2_scalar_mul")


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gpu_helpers
    gpu_helpers.amd.lib()
    return gpu_helpers.amd


def _multiples(group, n, seed):
    """n distinct multiples of a random point (tests/test_gpu_points.py _g1_points)"""
    rnd = random.Random(seed)
    mul, add, gen = (pr.g1_mul, pr.g1_add, pr.G1) if group == "g1" else (pr.g2_mul, pr.g2_add, pr.G2)
    base = mul(rnd.randrange(1, pr.R), gen)
    pts, acc = [], base
    for _ in range(n):
        pts.append(acc)
        acc = add(acc, base)
    return pts


@pytest.fixture(scope="module")
def g1_pts():
    return _multiples("g1", 320, 0x51)


@pytest.fixture(scope="module")
def g2_pts():
    return _multiples("g2", 2 * BLOCK + 1, 0x52)


def _enc(group, pts):
    enc = H.g1_affine_mont if group == "g1" else H.g2_affine_mont
    return np.array([enc(p) for p in pts], dtype=np.uint64).reshape(len(pts), 12 if group == "g1" else 24)


def _scalars(vals):
    return H.ints_to_limbs([int(v) for v in vals], 4)


def _check(amd, group, pts, scalars, raw):
    """raw (n, 18 | 36) Jacobian Montgomery == scalars[i] * pts[i] for every i"""
    mul = pr.g1_mul if group == "g1" else pr.g2_mul
    aff = amd.convert_points(group, "to_affine", np.ascontiguousarray(raw))
    zw = slice(12, 18) if group == "g1" else slice(24, 36)
    want = _enc(group, [None if p is None else mul(s % pr.R, p) for s, p in zip(scalars, pts)])
    for i in range(len(pts)):
        assert [int(v) for v in aff[i]] == [int(v) for v in want[i]], (group, i, hex(scalars[i]))
        if not want[i].any():
            assert not raw[i, zw].any(), (group, i, "identity must have Z = 0")


def _run(amd, group, pts, scalars, **kw):
    raw = amd.scalar_mul(group, _enc(group, pts), _scalars(scalars), **kw)
    _check(amd, group, pts, scalars, raw)
    return raw


def test_g1_edge_scalars(amd, g1_pts):
    lam, h, r = pr.GLV_LAMBDA, pr.GLV_LAMBDA >> 1, pr.R
    rnd = random.Random(0x61)
    sc = [0, 1, 2, r - 1, r, r + 1, (1 << 256) - 1, lam - 1, lam, lam + 1, h, h + 1, 7 * lam,
          (h + 5) * lam % r, ((h + 5) * lam + h + 9) % r]
    nwin = 128 // WINDOW
    # a single non-zero digit at every window position of the first half, then of the second
    sc += [1 << (WINDOW * w) for w in range(nwin)]
    sc += [(lam << (WINDOW * w)) % r for w in range(nwin)]
    # the recoding's extremes: 8 at position w is the digit -8 with +1 above it; 7 stays 7; a run
    # of 8s and of 7s through all positions below the top
    sc += [8 << (WINDOW * w) for w in range(nwin - 1)]
    sc += [7 << (WINDOW * w) for w in (0, nwin // 2, nwin - 2)]
    sc += [int("8" * (nwin - 1), 16), int("7" * (nwin - 1), 16), int("f" * (nwin - 1), 16),
           (int("8" * (nwin - 1), 16) * lam) % r]
    sc += [rnd.randrange(r) for _ in range(64)]
    for s, want in ((h, (h, False, 0)), (h + 1, (h, True, 1)), (7 * lam, (0, None, 7))):  # the issue's table
        m1, n1, m2, n2 = pr.glv_decompose(s)
        assert (m1, m2) == (want[0], want[2]) and (want[1] is None or n1 == want[1]), (s, m1, n1, m2, n2)
    assert len(sc) <= len(g1_pts)
    _run(amd, "g1", g1_pts[:len(sc)], sc)


def test_g1_identity_cases(amd, g1_pts):
    rnd = random.Random(0x62)
    pts = [None, None, g1_pts[3], g1_pts[4], g1_pts[5], None]
    sc = [rnd.randrange(1, pr.R), 1, 0, pr.R, rnd.randrange(1, pr.R), 0]
    raw = _run(amd, "g1", pts, sc)
    for i in (0, 1, 2, 3, 5):
        assert not raw[i, 12:18].any(), i
    assert raw[4, 12:18].any()


def test_g2_edge_scalars(amd, g2_pts):
    x, r = pr.PSI_X, pr.R
    rnd = random.Random(0x63)
    sc = [0, 1, r - 1, r, (1 << 256) - 1, x, x // 2 + 1, x * x, x ** 3 + x // 2 + 1, (x ** 4 - 1) % r]
    # the lowest and the highest bit of each of the four digits alone, and all four together
    sc += [(x ** j << b) % r for j in range(4) for b in (0, 62)]
    sc += [(1 + x + x * x + x ** 3) % r, ((1 + x + x * x + x ** 3) << 62) % r]
    sc += [rnd.randrange(r) for _ in range(24)]
    pts = g2_pts[:len(sc)] + [None, g2_pts[0], g2_pts[1]]
    sc += [rnd.randrange(1, r), 0, r]
    raw = _run(amd, "g2", pts, sc)
    for i in (len(sc) - 3, len(sc) - 2, len(sc) - 1):
        assert not raw[i, 24:36].any(), i


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2 * BLOCK + 1])
def test_g1_sizes(amd, g1_pts, n):
    rnd = random.Random(0x70 + n)
    _run(amd, "g1", g1_pts[:n], [rnd.randrange(pr.R) for _ in range(n)])


@pytest.mark.parametrize("n", [1, 65, 2 * BLOCK + 1])
def test_g2_sizes(amd, g2_pts, n):
    rnd = random.Random(0x80 + n)
    _run(amd, "g2", g2_pts[:n], [rnd.randrange(pr.R) for _ in range(n)])


def test_placement_combinations(amd, g1_pts):
    """all eight host / device placements of bases, scalars and output give the same bytes"""
    import torch
    n = 65
    rnd = random.Random(0x90)
    pts, sc = g1_pts[:n], [rnd.randrange(pr.R) for _ in range(n)]
    b, s = _enc("g1", pts), _scalars(sc)
    ref = amd.scalar_mul("g1", b, s)
    _check(amd, "g1", pts, sc, ref)
    for bd in (False, True):
        for sd in (False, True):
            for od in (False, True):
                out = torch.zeros((n, 18), dtype=torch.int64, device="cuda") if od else None
                got = amd.scalar_mul("g1", amd.torch_u64(b) if bd else b, amd.torch_u64(s) if sd else s, out=out)
                got = amd.to_numpy_u64(got) if od else got
                assert np.array_equal(got, ref), (bd, sd, od)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_montgomery_scalars(amd, g1_pts, g2_pts, group):
    n = 65 if group == "g1" else 9
    rnd = random.Random(0xA0)
    pts = (g1_pts if group == "g1" else g2_pts)[:n]
    sc = [rnd.randrange(pr.R) for _ in range(n - 3)] + [0, 1, pr.R - 1]
    std = _run(amd, group, pts, sc)
    mont = amd.scalar_mul(group, _enc(group, pts), _scalars([pr.fr_to_mont(v) for v in sc]), scalars_mont=True)
    assert np.array_equal(mont, std)


def _raw_call(amd, name, b, s, n, cfg, out, mont=None):
    fn = getattr(amd.lib(), name)
    if name.startswith("mbls_"):
        return fn(amd._p(b), amd._p(s), n, bool(mont), ctypes.byref(cfg) if cfg is not None else None, amd._p(out))
    return fn(amd._p(b), amd._p(s), n, ctypes.byref(cfg) if cfg is not None else None, amd._p(out))


def test_glv_entry_and_standard_entries(amd, g1_pts, g2_pts):
    """bls12_381_g1_scalar_mul, its _glv twin and bls12_381_g2_scalar_mul give the bytes of the
    mbls_* forms on standard scalars"""
    rnd = random.Random(0xB0)
    for group, pts, names in (("g1", g1_pts[:65], ENTRIES[:2]), ("g2", g2_pts[:5], ENTRIES[2:3])):
        n = len(pts)
        sc = [rnd.randrange(1 << 256) for _ in range(n)]
        ref = _run(amd, group, pts, sc)
        b, s = _enc(group, pts), _scalars(sc)
        for name in names:
            out = np.zeros_like(ref)
            assert _raw_call(amd, name, b, s, n, amd.vec_config(), out) == amd.SUCCESS
            assert np.array_equal(out, ref), name


def test_async_on_a_side_stream(amd, g1_pts):
    import torch
    n = 65
    rnd = random.Random(0xC0)
    pts, sc = g1_pts[:n], [rnd.randrange(pr.R) for _ in range(n)]
    b, s = amd.torch_u64(_enc("g1", pts)), amd.torch_u64(_scalars(sc))
    sync = torch.zeros((n, 18), dtype=torch.int64, device="cuda")
    amd.scalar_mul("g1", b, s, out=sync)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    out = torch.zeros((n, 18), dtype=torch.int64, device="cuda")
    amd.scalar_mul("g1", b, s, out=out, stream=st, is_async=True)
    st.synchronize()
    assert torch.equal(out, sync)
    _check(amd, "g1", pts, sc, amd.to_numpy_u64(sync))
    amd.release_stream(st)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_many_workgroups_against_the_msm(amd, group):
    """n = 2^12 + 3 device-generated pairs: the sum of the products equals the raw MSM"""
    import torch
    n = (1 << 12) + 3
    nl = 12 if group == "g1" else 24
    s = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    b = torch.zeros((n, nl), dtype=torch.int64, device="cuda")
    amd.gen_scalars(s, 0x5CA1A1, montgomery=False)
    amd.gen_bases(group, b, 0x5CA1A2)
    prod = torch.zeros((n, nl * 3 // 2), dtype=torch.int64, device="cuda")
    amd.scalar_mul(group, b, s, out=prod)
    tot = torch.zeros((1, nl * 3 // 2), dtype=torch.int64, device="cuda")
    amd.sum_jacobian(group, prod, tot)
    torch.cuda.synchronize()
    want = amd.msm(group, s, b, icicle=False)
    got_aff = amd.convert_points(group, "to_affine", amd.to_numpy_u64(tot))
    want_aff = amd.convert_points(group, "to_affine", want)
    assert got_aff.any()
    assert np.array_equal(got_aff, want_aff)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_more_than_one_launch(amd, group):
    """a batch past the per-launch lane limit (SM_G1_CHUNK / SM_G2_CHUNK) runs as several
    launches over one table: the pairs on both sides of the boundary and at the end give the
    bytes of the same pairs run as small batches (the path the pyref tests pin)"""
    import torch
    chunk = (1 << 18) if group == "g1" else (1 << 16)
    n = chunk + 5
    nl = 12 if group == "g1" else 24
    s = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    b = torch.zeros((n, nl), dtype=torch.int64, device="cuda")
    amd.gen_scalars(s, 0x5CA1B1, montgomery=False)
    amd.gen_bases(group, b, 0x5CA1B2)
    full = torch.zeros((n, nl * 3 // 2), dtype=torch.int64, device="cuda")
    amd.scalar_mul(group, b, s, out=full)
    for lo, hi in ((0, 64), (chunk - 64, chunk), (chunk, n)):
        part = torch.zeros((hi - lo, nl * 3 // 2), dtype=torch.int64, device="cuda")
        amd.scalar_mul(group, b[lo:hi].contiguous(), s[lo:hi].contiguous(), out=part)
        assert torch.equal(part, full[lo:hi]), (group, lo, hi)
        assert bool(part.any(dim=1).all())


def test_no_allocation_after_warm_up(amd, g1_pts):
    n = 65
    rnd = random.Random(0xD0)
    b, s = _enc("g1", g1_pts[:n]), _scalars([rnd.randrange(pr.R) for _ in range(n)])
    first = amd.scalar_mul("g1", b, s)
    m0, f0 = amd.scratch_stats()[:2]
    second = amd.scalar_mul("g1", b, s)
    m1, f1 = amd.scratch_stats()[:2]
    assert (m1, f1) == (m0, f0)
    assert np.array_equal(first, second)


def test_argument_errors(amd):
    cfg = amd.vec_config()
    buf = np.zeros((4, 36), dtype=np.uint64)
    for name in ENTRIES:
        def call(b=buf, s=buf, n=4, c=cfg, o=buf):
            return _raw_call(amd, name, b, s, n, c, o, mont=False)
        assert call(b=None) == amd.INVALID_ARGUMENT, name
        assert call(s=None) == amd.INVALID_ARGUMENT, name
        assert call(o=None) == amd.INVALID_ARGUMENT, name
        assert call(c=None) == amd.INVALID_ARGUMENT, name
        assert call(n=0) == amd.INVALID_ARGUMENT, name
        assert call(n=-1) == amd.INVALID_ARGUMENT, name
        assert call(n=(1 << 26) + 1) == amd.INVALID_ARGUMENT, name
