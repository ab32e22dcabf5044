"""Batch point validation (mbls_g1_check_points / mbls_g2_check_points) on the GPU against the
definition taken on the CPU (tests/subgroup_cases.py): canonical words, the curve equation, and
[r]P == O by an unreduced double-and-add, computed once per distinct point.  Membership is decided
exactly on both sides: every status byte and every count is compared for equality."""
import ctypes
import random

import numpy as np
import pytest

import subgroup_cases as S
from helpers import pyref as pr

pytestmark = pytest.mark.gpu

BLOCK = 64  # lanes per workgroup (SM_BLOCK): one wave
WAVE = {"g1": BLOCK, "g2": BLOCK // 2}  # points per wave: a G2 point lives in a pair of lanes
GROUPS = ["g1", "g2"]
SIZES = [(g, n) for g in GROUPS
         for n in sorted({1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1} | {WAVE[g] - 1, WAVE[g], WAVE[g] + 1})]


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gpu_helpers
    gpu_helpers.amd.lib()
    return gpu_helpers.amd


def _invalid_cases(group):
    """the distinct invalid cases larger batches repeat: every on-curve non-member, then one of
    each cheaper status"""
    t = S.status_table(group)
    return [S.case(group, p) for p in S.non_members(group)] + list(t[4:8])


def _run(amd, group, cases, **kw):
    """status and count of one call, checked against the definition"""
    want = np.array([S.expected(group, c) for c in cases], dtype=np.uint8)
    st, cnt = amd.check_points(group, S.encode(group, cases), **kw)
    assert st.dtype == np.uint8 and st.shape == (len(cases),)
    assert [int(v) for v in st] == [int(v) for v in want], group
    assert cnt == int((want >= 2).sum())
    return want


@pytest.mark.parametrize("group", GROUPS)
def test_status_table(amd, group):
    cases = S.status_table(group)
    want = _run(amd, group, cases)
    # the rows the table must hold, by the definition (no case may be missing)
    assert list(want[:8]) == [S.OK, S.OK, S.OK, S.IDENTITY, S.NONCANONICAL, S.NONCANONICAL, S.OFF_CURVE, S.OFF_CURVE]
    nm = S.non_members(group)
    assert len(cases) == 8 + len(nm) and all(w == S.OFF_SUBGROUP for w in want[8:])
    for p in list(S.torsion_points(group)) + list(S.member_plus_torsion(group)) + list(S.random_curve_points(group, 8)):
        assert p in nm
    if group == "g1":
        assert (0, 2) in nm and (0, pr.P - 2) in nm
    else:
        assert any(p[0][1] == 0 for p in nm)


@pytest.mark.parametrize("group,n", SIZES)
def test_lane_and_wave_boundaries(amd, group, n):
    """an invalid point first, last and on each side of every wave boundary, members in between"""
    bad = _invalid_cases(group)
    cases = [S.case(group, p) for p in S.members(group, 2 * BLOCK + 1)[:n]]
    spots = sorted({0, n - 1} | {k for b in range(WAVE[group], n, WAVE[group]) for k in (b - 1, b)})
    for j, k in enumerate(spots):
        cases[k] = bad[(7 * n + j) % len(bad)]
    want = _run(amd, group, cases)
    assert all(want[k] >= 2 for k in spots) and int((want >= 2).sum()) == len(spots)


@pytest.mark.parametrize("group", GROUPS)
def test_count_across_waves(amd, group):
    rnd = random.Random(0xC0 + len(group))
    bad, good = _invalid_cases(group), [S.case(group, p) for p in S.members(group, 2 * BLOCK + 1)]
    good.append(S.case(group, None))
    n = 1003
    cases = [rnd.choice(bad) if rnd.random() < 0.5 else rnd.choice(good) for _ in range(n)]
    want = _run(amd, group, cases)
    assert 400 < int((want >= 2).sum()) < 600
    # the count alone, and the statuses alone
    st, cnt = amd.check_points(group, S.encode(group, cases), out=False)
    assert st is None and cnt == int((want >= 2).sum())
    st, cnt = amd.check_points(group, S.encode(group, cases), count=False)
    assert cnt is None and np.array_equal(st, want)


@pytest.mark.parametrize("group", GROUPS)
def test_forms_and_placement(amd, group):
    import torch
    cases = S.status_table(group)
    n = len(cases)
    want = np.array([S.expected(group, c) for c in cases], dtype=np.uint8)
    bad = int((want >= 2).sum())
    mont, std = S.encode(group, cases), S.encode(group, cases, mont=False)
    for words, pm in ((mont, True), (std, False)):
        st, cnt = amd.check_points(group, words, points_mont=pm)
        assert np.array_equal(st, want) and cnt == bad, pm
        dev = amd.torch_u64(words)
        st, cnt = amd.check_points(group, dev, points_mont=pm)                      # device points, host status
        assert np.array_equal(st, want) and cnt == bad, pm
        for pts in (words, dev):                                                    # device status
            out = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
            got, cnt = amd.check_points(group, pts, points_mont=pm, out=out)
            assert got is out and cnt == bad
            assert np.array_equal(out.cpu().numpy(), want), pm
        st, cnt = amd.check_points(group, dev, points_mont=pm, out=False)           # a count only
        assert st is None and cnt == bad
        out = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        got, cnt = amd.check_points(group, dev, points_mont=pm, out=out, count=False)  # statuses only
        torch.cuda.synchronize()
        assert cnt is None and np.array_equal(out.cpu().numpy(), want)
    # asynchronous on a side stream: device points and status, no count, then a stream synchronise
    side = torch.cuda.Stream()
    dev = amd.torch_u64(mont)
    out = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    amd.check_points(group, dev, out=out, count=False, stream=side, is_async=True)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    # is_async with a count: the count is a host output, so the call has finished on return
    out = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    _, cnt = amd.check_points(group, dev, out=out, stream=side, is_async=True)
    assert cnt == bad
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    amd.release_stream(side)


@pytest.mark.parametrize("group", GROUPS)
def test_argument_errors(amd, group):
    fn = getattr(amd.lib(), "mbls_g1_check_points" if group == "g1" else "mbls_g2_check_points")
    cfg = amd.vec_config()
    pts = S.encode(group, [S.case(group, p) for p in S.members(group, 4)])
    status = np.full(4, 0xAA, dtype=np.uint8)
    cnt = ctypes.c_uint64(0xDEADBEEF)

    def call(p=pts, n=4, c=cfg, st=status, k=cnt):
        return fn(amd._p(p), n, True, ctypes.byref(c) if c is not None else None, amd._p(st),
                  ctypes.byref(k) if k is not None else None)

    assert call(p=None) == amd.INVALID_ARGUMENT
    assert call(c=None) == amd.INVALID_ARGUMENT
    assert call(st=None, k=None) == amd.INVALID_ARGUMENT
    assert call(n=0) == amd.INVALID_ARGUMENT
    assert call(n=-1) == amd.INVALID_ARGUMENT
    assert call(n=(1 << 26) + 1) == amd.INVALID_ARGUMENT
    assert (status == 0xAA).all() and cnt.value == 0xDEADBEEF  # the outputs stay untouched
    assert call() == amd.SUCCESS
    assert (status == S.OK).all() and cnt.value == 0


@pytest.mark.parametrize("group", GROUPS)
def test_consistent_with_scalar_mul(amd, group):
    """members only: status OK coincides with scalar_mul(r - 1, P) == -P from the existing entry"""
    import helpers as H
    n = BLOCK + 1 if group == "g1" else 9
    pts = S.members(group, 2 * BLOCK + 1)[:n]
    neg = S.ops(group)[1]
    words = S.encode(group, [S.case(group, p) for p in pts])
    st, cnt = amd.check_points(group, words)
    assert (st == S.OK).all() and cnt == 0
    sc = H.ints_to_limbs([pr.R - 1] * n, 4)
    aff = amd.convert_points(group, "to_affine", amd.scalar_mul(group, words, sc))
    assert np.array_equal(aff, S.encode(group, [S.case(group, neg(p)) for p in pts]))
