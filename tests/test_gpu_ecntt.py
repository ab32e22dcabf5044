"""G1 EC-NTT (mbls_g1_ecntt) on the GPU.

Expected values need no EC-NTT on the CPU: inputs are P_i = [k_i] G with known standard-form k_i,
the transform is linear, so out_j = [NTT(k)_j] G -- the oracle's Fr NTT (orc_ntt, applied to the
standard-form limbs: its Montgomery products by Montgomery twiddles keep them standard) and one
orc_g1_mul_gen per element give the affine Montgomery bytes.  Every element of every output is
compared byte for byte (the output is canonical affine); the 2^20 case, whose expected values would
cost a million CPU multiplications, is pinned by the exact round trip and by the library's MSM at
four output indices instead."""
import ctypes
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import helpers as H
from helpers import pyref as pr

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 4, 8, 16, 64, 128, 256, 2048)
CHUNK = 1 << 18  # butterflies per launch (SM_G1_CHUNK)


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gpu_helpers
    gpu_helpers.amd.lib()
    return gpu_helpers.amd


def _mul_gen(ks):
    """[k] G for standard-form ints k -> (n, 12) affine Montgomery limbs (orc_g1_mul_gen per element)"""
    o = H.oracle()
    n = len(ks)
    sc = H.ints_to_limbs([int(k) for k in ks], 4)
    out = np.zeros((n, 12), dtype=np.uint64)

    def run(lo):
        for i in range(lo, min(lo + 64, n)):
            o.orc_g1_mul_gen(out[i].ctypes.data, sc[i].ctypes.data)
    with ThreadPoolExecutor(8) as ex:  # ctypes drops the GIL for the call
        list(ex.map(run, range(0, n, 64)))
    return out


def _ntt_std(ks, inverse):
    """the Fr NTT of standard-form ints (orc_ntt is linear: standard in, standard out)"""
    n = len(ks)
    log_n = n.bit_length() - 1
    assert 1 << log_n == n
    return H.limbs_to_ints(H.oracle_ntt(H.ints_to_limbs([int(k) % pr.R for k in ks], 4), log_n, inverse))


def _expected(ks, inverse):
    return _mul_gen(_ntt_std(ks, inverse))


def _check(amd, ks, inverse, pts=None):
    """transform [k_i] G and compare every output element's bytes with [NTT(k)_j] G"""
    pts = _mul_gen(ks) if pts is None else pts
    got = amd.ecntt(pts, inverse=inverse)
    want = _expected(ks, inverse)
    assert got.shape == want.shape
    for j in range(len(ks)):
        assert got[j].tobytes() == want[j].tobytes(), (len(ks), inverse, j)
    return got


@pytest.fixture(scope="module")
def stream():
    """2048 oracle-generated pairs (k_i standard form, P_i = [k_i] G) of one seed"""
    o = H.oracle()
    n = SIZES[-1]
    ks = np.zeros((n, 4), dtype=np.uint64)
    pts = np.zeros((n, 12), dtype=np.uint64)
    o.orc_gen_scalars(H.ptr(ks), 0xEC17, n)
    o.orc_gen_g1_bases(H.ptr(pts), 0xEC17, n, 0)
    ints = H.limbs_to_ints(ks)
    assert np.array_equal(_mul_gen(ints[:2]), pts[:2])  # the two generators agree on the stream
    return ints, pts


def test_mul_gen_of_zero_is_the_all_zero_point():
    assert not _mul_gen([0]).any()


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(amd, stream, n, inverse):
    ks, pts = stream
    _check(amd, ks[:n], inverse, np.ascontiguousarray(pts[:n]))


@pytest.mark.parametrize("n", [8, 64])
def test_all_inputs_equal(amd, n):
    """a = t in stage 1 (madd's doubling branch), identities from then on"""
    c = random.Random(0xE1 + n).randrange(1, pr.R)
    got = _check(amd, [c] * n, False)
    assert got[0].any() and not got[1:].any()
    assert np.array_equal(got[:1], _mul_gen([n * c % pr.R]))
    _check(amd, [c] * n, True)


@pytest.mark.parametrize("n", [8, 64])
def test_single_non_identity_input(amd, n):
    """k = (c, 0, ..., 0): an identity b operand in every stage"""
    c = random.Random(0xE2 + n).randrange(1, pr.R)
    ks = [c] + [0] * (n - 1)
    got = _check(amd, ks, False)
    assert np.array_equal(got, np.repeat(_mul_gen([c]), n, axis=0))
    _check(amd, ks, True)


@pytest.mark.parametrize("m_of", ["1", "n/2+1"])
@pytest.mark.parametrize("n", [8, 64])
def test_exact_cancellation(amd, n, m_of):
    """k_i = c w^(-i m): a = -t meets non-trivial twiddles; the output is non-zero only at index m"""
    m = 1 if m_of == "1" else n // 2 + 1
    c = random.Random(0xE3 + n + m).randrange(1, pr.R)
    wi = pow(pr.omega(n.bit_length() - 1), -1, pr.R)
    ks = [c * pow(wi, i * m, pr.R) % pr.R for i in range(n)]
    got = _check(amd, ks, False)
    assert got[m].any() and not np.delete(got, m, axis=0).any()
    _check(amd, ks, True)


@pytest.mark.parametrize("n", [8, 64])
def test_identities_among_random_points(amd, n):
    rnd = random.Random(0xE4 + n)
    ks = [0 if rnd.random() < 0.4 else rnd.randrange(1, pr.R) for _ in range(n)]
    ks[0], ks[n // 2] = 0, rnd.randrange(1, pr.R)  # a = identity against a live b in stage 1
    assert 0 < sum(k == 0 for k in ks) < n
    for inverse in (False, True):
        _check(amd, ks, inverse)


def _device_bases(amd, n, seed):
    import torch
    b = torch.zeros((n, 12), dtype=torch.int64, device="cuda")
    amd.gen_bases("g1", b, seed)
    return b


def test_round_trip(amd):
    import torch
    n = 1 << 12
    p = _device_bases(amd, n, 0xEC18)
    f = torch.zeros_like(p)
    back = torch.zeros_like(p)
    amd.ecntt(p, out=f)
    amd.ecntt(f, inverse=True, out=back)
    assert bool(p.any(dim=1).all())
    assert not torch.equal(f, p)
    assert torch.equal(back, p)


def _powers_std(o, base, n):
    """(base^i) for i < n as standard-form limbs, by doubling with the oracle's vector products
    (a standard-form vector times a Montgomery scalar stays standard)"""
    out = np.zeros((n, 4), dtype=np.uint64)
    out[0, 0] = 1
    m = 1
    while m < n:
        mult = H.ints_to_limbs([pr.fr_to_mont(pow(base, m, pr.R))], 4)
        o.orc_scalar_mul_vec(H.ptr(out[m:2 * m]), H.ptr(mult), H.ptr(out[:m]), m)
        m *= 2
    return out


def test_more_than_one_launch_per_stage(amd):
    """n = 2^20: n/2 butterflies exceed the 2^18 lanes of one launch"""
    import torch
    n = 1 << 20
    assert n // 2 > CHUNK and n // 4 <= CHUNK
    o = H.oracle()
    p = _device_bases(amd, n, 0xEC19)
    f = torch.zeros_like(p)
    back = torch.zeros_like(p)
    amd.ecntt(p, out=f)
    amd.ecntt(f, inverse=True, out=back)
    assert torch.equal(back, p)
    w = pr.omega(20)
    seeded = random.Random(0xEC1A).randrange(2, n)
    # the doubling above is pinned against plain powers at a few places
    chk = _powers_std(o, pow(w, seeded, pr.R), n)
    for i in (0, 1, 2, 12345, n - 1):
        assert H.limbs_to_ints(chk[i])[0] == pow(w, seeded * i, pr.R)
    fh = amd.to_numpy_u64(f)
    for j in (0, 1, n // 2, seeded):
        sc = chk if j == seeded else _powers_std(o, pow(w, j, pr.R), n)
        raw = amd.msm("g1", amd.torch_u64(sc), p, icicle=False)
        want = amd.convert_points("g1", "to_affine", raw)
        assert want.any(), j
        assert fh[j].tobytes() == want[0].tobytes(), j
    jac = torch.zeros((n, 18), dtype=torch.int64, device="cuda")
    amd.convert_points("g1", "to_projective", p, out=jac)
    tot = torch.zeros((1, 18), dtype=torch.int64, device="cuda")
    amd.sum_jacobian("g1", jac, tot)
    torch.cuda.synchronize()
    assert fh[0].tobytes() == amd.convert_points("g1", "to_affine", amd.to_numpy_u64(tot))[0].tobytes()


def test_monomial_srs_to_lagrange_commitments(amd):
    """g_j = [s^j] G -> gl = inverse EC-NTT = [L_i(s)] G; a commitment to coefficients c against g
    equals the commitment to the evaluations NTT(c) against gl"""
    import gpu_helpers
    n, log_n = 1 << 10, 10
    rnd = random.Random(0xEC1B)
    s = rnd.randrange(2, pr.R)
    ks = [pow(s, j, pr.R) for j in range(n)]
    g = _mul_gen(ks)
    gl = _check(amd, ks, True, g)
    c = [rnd.randrange(pr.R) for _ in range(n)]
    ev = _ntt_std(c, False)
    a = amd.msm("g1", H.ints_to_limbs(c, 4), g)
    b = amd.msm("g1", H.ints_to_limbs(ev, 4), gl)
    assert gpu_helpers.decode_icicle("g1", a[0]) is not None
    assert np.array_equal(a, b)


def test_placement_combinations(amd, stream):
    """host / device input and output, and input == output on the device, give the same bytes"""
    import torch
    ks, pts = stream
    n = 128
    h = np.ascontiguousarray(pts[:n])
    for inverse in (False, True):
        ref = _check(amd, ks[:n], inverse, h)
        for ind in (False, True):
            for outd in (False, True):
                out = torch.zeros((n, 12), dtype=torch.int64, device="cuda") if outd else None
                got = amd.ecntt(amd.torch_u64(h) if ind else h, inverse=inverse, out=out)
                got = amd.to_numpy_u64(got) if outd else got
                assert np.array_equal(got, ref), (inverse, ind, outd)
        same = amd.torch_u64(h)
        amd.ecntt(same, inverse=inverse, out=same)
        assert np.array_equal(amd.to_numpy_u64(same), ref), (inverse, "in place")


def test_async_on_a_side_stream(amd, stream):
    import torch
    ks, pts = stream
    n = 128
    p = amd.torch_u64(np.ascontiguousarray(pts[:n]))
    sync = torch.zeros_like(p)
    amd.ecntt(p, inverse=True, out=sync)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    out = torch.zeros_like(p)
    amd.ecntt(p, inverse=True, out=out, stream=st, is_async=True)
    st.synchronize()
    assert torch.equal(out, sync)
    assert np.array_equal(amd.to_numpy_u64(sync), _expected(ks[:n], True))
    amd.release_stream(st)


def test_no_allocation_after_warm_up(amd, stream):
    _, pts = stream
    h = np.ascontiguousarray(pts[:128])
    first = amd.ecntt(h, inverse=True)
    m0, f0 = amd.scratch_stats()[:2]
    second = amd.ecntt(h, inverse=True)
    m1, f1 = amd.scratch_stats()[:2]
    assert (m1, f1) == (m0, f0)
    assert np.array_equal(first, second)


def _raw(amd, inp, n, cfg, out, d=0):
    return amd.lib().mbls_g1_ecntt(amd._p(inp), n, d, ctypes.byref(cfg) if cfg is not None else None, amd._p(out))


def test_argument_errors(amd):
    buf = np.zeros((128, 12), dtype=np.uint64)
    out = np.zeros_like(buf)
    ok = amd.ntt_config()
    assert _raw(amd, buf, 8, ok, out) == amd.SUCCESS
    assert _raw(amd, None, 8, ok, out) == amd.INVALID_POINTER
    assert _raw(amd, buf, 8, ok, None) == amd.INVALID_POINTER
    assert _raw(amd, buf, 8, None, out) == amd.INVALID_POINTER
    for size in (0, -1, 3, 96, (1 << 26) + 1):
        assert _raw(amd, buf, size, ok, out) == amd.INVALID_ARGUMENT, size
    assert _raw(amd, buf, 8, amd.ntt_config(batch_size=2), out) == amd.INVALID_ARGUMENT
    assert _raw(amd, buf, 8, amd.ntt_config(batch_size=0), out) == amd.SUCCESS
    assert _raw(amd, buf, 8, amd.ntt_config(columns_batch=True), out) == amd.INVALID_ARGUMENT
    for name, val in amd.ORDERINGS.items():
        want = amd.SUCCESS if name == "NN" else amd.INVALID_ARGUMENT
        assert _raw(amd, buf, 8, amd.ntt_config(ordering=val), out) == want, name
    assert _raw(amd, buf, 8, amd.NTTConfig(), out) == amd.INVALID_ARGUMENT  # zero-initialised: coset_gen 0
    assert _raw(amd, buf, 8, amd.ntt_config(coset_gen=[0, 0, 0, 0]), out) == amd.INVALID_ARGUMENT
    seven = pr.int_to_limbs(pr.fr_to_mont(7), 4)
    assert _raw(amd, buf, 8, amd.ntt_config(coset_gen=seven), out) == amd.INVALID_ARGUMENT
    assert _raw(amd, buf, 8, amd.ntt_config(coset_gen=pr.int_to_limbs(1, 4)), out) == amd.INVALID_ARGUMENT


def test_domain_order_bounds_the_size(amd):
    buf = np.zeros((16, 12), dtype=np.uint64)
    out = np.zeros_like(buf)
    cfg = amd.ntt_config()
    try:
        w8 = pr.int_to_limbs(pr.fr_to_mont(pr.omega(3)), 4)
        amd.ntt_init_domain(np.array(w8, dtype=np.uint64))
        assert _raw(amd, buf, 8, cfg, out) == amd.SUCCESS
        assert _raw(amd, buf, 16, cfg, out) == amd.INVALID_ARGUMENT
    finally:
        amd.ntt_init_domain()
    assert _raw(amd, buf, 16, cfg, out) == amd.SUCCESS
