"""Batch point compression / decompression (mbls_g*_compress, mbls_g*_decompress) on the GPU against
the format's model on the CPU (tests/serde_model.py: pure-Python integers and roots).  Every
comparison is exact equality: status bytes, counts, point words and record bytes."""
import ctypes
import functools
import random

import numpy as np
import pytest

import serde_model as M
import subgroup_cases as S
from helpers import pyref as pr

pytestmark = pytest.mark.gpu

BLOCK = 64  # lanes per workgroup (SM_BLOCK): one wave
WAVE = {"g1": BLOCK, "g2": BLOCK // 2}  # records per wave: a G2 point lives in a pair of lanes
GROUPS = ["g1", "g2"]
NL = {"g1": 12, "g2": 24}
SIZES = [(g, n) for g in GROUPS for n in sorted({1, 63, 64, 65, 129} | ({31, 32, 33} if g == "g2" else set()))]


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gpu_helpers
    gpu_helpers.amd.lib()
    return gpu_helpers.amd


@functools.lru_cache(maxsize=None)
def _decode(group, rec):
    return M.decode(group, rec)


def _model(group, records):
    out = [_decode(group, r) for r in records]
    return np.array([s for s, _ in out], dtype=np.uint8), [p for _, p in out]


@functools.lru_cache(maxsize=None)
def _member_records(group):
    """records of 129 members, every second one negated so that both S values occur"""
    neg = S.ops(group)[1]
    return tuple(M.encode(group, neg(p) if k & 1 else p) for k, p in enumerate(S.members(group, 2 * BLOCK + 1)))


def _dev(a):
    import torch
    return torch.from_numpy(a).cuda()


def _check(amd, group, records, mont=True, **kw):
    """one decompress call against the model: statuses, count, points (zeroed where invalid)"""
    want_st, want_pts = _model(group, records)
    pts, st, cnt = amd.decompress_points(group, M.to_array(group, records), points_mont=mont, **kw)
    assert st.dtype == np.uint8 and st.shape == (len(records),)
    assert [int(v) for v in st] == [int(v) for v in want_st], group
    assert cnt == int((want_st >= 2).sum())
    assert pts.shape == (len(records), NL[group])
    assert np.array_equal(pts, M.words(group, want_pts, mont=mont)), group
    return want_st, want_pts


@pytest.mark.parametrize("mont", [True, False])
@pytest.mark.parametrize("group", GROUPS)
def test_status_and_value_table(amd, group, mont):
    records, st, pts = M.status_table(group)
    assert records[0].hex() == (M.G1_HEX if group == "g1" else M.G2_HEX)
    want_st, want_pts = _check(amd, group, list(records), mont=mont)
    assert np.array_equal(want_st, st) and tuple(want_pts) == pts
    gen, last = pts[0], pts[1]
    assert gen == S.ops(group)[3] and last == S.ops(group)[1](gen)
    n_valid = 2 + 12 + len(M.g1_specials() if group == "g1" else M.g2_specials())
    assert all(s == M.OK for s in st[:n_valid]) and st[n_valid] == M.IDENTITY
    assert [int(s) for s in st[n_valid + 1:]] == [s for _, s in M.malformed(group)]
    # the table compresses back to itself on its valid records, in either form
    back = amd.compress_points(group, M.words(group, want_pts, mont=mont), points_mont=mont)
    for k, rec in enumerate(records):
        assert bytes(back[k]) == (rec if st[k] == M.OK else M.infinity(group)), k


@pytest.mark.parametrize("group,n", SIZES)
def test_lane_pair_and_wave_boundaries(amd, group, n):
    """an invalid record first, last and on each side of every wave boundary, members in between"""
    bad = [r for r, s in M.malformed(group) if s >= 2]
    records = list(_member_records(group)[:n])
    spots = sorted({0, n - 1} | {k for b in range(WAVE[group], n, WAVE[group]) for k in (b - 1, b)})
    for j, k in enumerate(spots):
        records[k] = bad[(7 * n + j) % len(bad)]
    want_st, want_pts = _check(amd, group, records)
    assert all(want_st[k] >= 2 for k in spots) and int((want_st >= 2).sum()) == len(spots)
    assert all(want_pts[k] is None for k in spots)


@pytest.mark.parametrize("group", GROUPS)
def test_round_trip(amd, group):
    import gpu_helpers
    rnd = random.Random(0x5E4D10 + len(group))
    n = 1003
    good, bad = _member_records(group), [r for r, _ in M.malformed(group)]
    records = []
    for _ in range(n):
        u = rnd.random()
        records.append(rnd.choice(bad) if u < 0.10 else M.infinity(group) if u < 0.15 else rnd.choice(good))
    want_st, want_pts = _check(amd, group, records)
    assert 60 < int((want_st >= 2).sum()) < 140 and int((want_st == M.IDENTITY).sum()) > 20
    data = M.to_array(group, records)
    # compress(decompress(bytes)) == bytes on the valid records (a rejected record comes back as infinity)
    pts, st, _ = amd.decompress_points(group, data)
    back = amd.compress_points(group, pts)
    assert back.dtype == np.uint8 and back.shape == data.shape
    valid = want_st < 2
    assert np.array_equal(back[valid], data[valid])
    assert all(bytes(r) == M.infinity(group) for r in back[~valid])
    # decompress(compress(points)) == points
    again, st2, cnt2 = amd.decompress_points(group, back)
    assert np.array_equal(again, pts) and cnt2 == 0
    assert np.array_equal(st2, np.where(valid, want_st, M.IDENTITY))
    # the decompressed members pass the validation
    members = np.ascontiguousarray(pts[want_st == M.OK])
    cst, cbad = amd.check_points(group, members)
    assert cbad == 0 and (cst == amd.POINT_OK).all()
    # and serve as device bases of an MSM
    k = 65
    dev_pts, _, _ = amd.decompress_points(group, _dev(np.ascontiguousarray(data[want_st == M.OK][:k])),
                                          out=amd.torch_u64((k, NL[group])), status=False)
    scalars = [rnd.randrange(pr.R) for _ in range(k)]
    import helpers as H
    got = amd.msm(group, H.ints_to_limbs(scalars, 4), dev_pts)
    model_pts = [p for p, s in zip(want_pts, want_st) if s == M.OK][:k]
    assert gpu_helpers.decode_icicle(group, got[0]) == pr.msm(scalars, model_pts, group)


@pytest.mark.parametrize("group", GROUPS)
def test_forms_and_placement(amd, group):
    import torch
    records, want_st, want_pts = M.status_table(group)
    n = len(records)
    bad = int((want_st >= 2).sum())
    data = M.to_array(group, list(records))
    ddata = _dev(data)

    def fresh():
        return (torch.full((n, NL[group]), 0x6E, dtype=torch.int64, device="cuda"),
                torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda"))

    for pm in (True, False):
        words = M.words(group, want_pts, mont=pm)
        recs = amd.compress_points(group, words, points_mont=pm)                     # host -> host
        for src in (data, ddata):                                                    # host outputs
            pts, st, cnt = amd.decompress_points(group, src, points_mont=pm)
            assert np.array_equal(pts, words) and np.array_equal(st, want_st) and cnt == bad, pm
            pts, st, cnt = amd.decompress_points(group, src, points_mont=pm, status=False)
            assert st is None and np.array_equal(pts, words) and cnt == bad
            pts, st, cnt = amd.decompress_points(group, src, points_mont=pm, count=False)
            assert cnt is None and np.array_equal(pts, words) and np.array_equal(st, want_st)
            pts, st, cnt = amd.decompress_points(group, src, points_mont=pm, status=False, count=False)
            assert st is None and cnt is None and np.array_equal(pts, words)
        for src in (data, ddata):                                                    # device outputs
            out, dst = fresh()
            pts, st, cnt = amd.decompress_points(group, src, points_mont=pm, out=out, status=dst)
            assert pts is out and st is dst and cnt == bad
            assert np.array_equal(amd.to_numpy_u64(out), words) and np.array_equal(dst.cpu().numpy(), want_st)
            out, dst = fresh()
            pts, st, cnt = amd.decompress_points(group, src, points_mont=pm, out=out, status=False)
            assert st is None and cnt == bad and np.array_equal(amd.to_numpy_u64(out), words)
            out, dst = fresh()
            amd.decompress_points(group, src, points_mont=pm, out=out, status=dst, count=False)
            torch.cuda.synchronize()
            assert np.array_equal(amd.to_numpy_u64(out), words) and np.array_equal(dst.cpu().numpy(), want_st)
        # compress: host / device points, host / device bytes
        dwords = amd.torch_u64(words)
        assert np.array_equal(amd.compress_points(group, dwords, points_mont=pm), recs)
        for src in (words, dwords):
            dbytes = torch.full((n, M.SIZE[group]), 0xEE, dtype=torch.uint8, device="cuda")
            assert amd.compress_points(group, src, points_mont=pm, out=dbytes) is dbytes
            assert np.array_equal(dbytes.cpu().numpy(), recs)
    # asynchronous on a side stream: device everything, no count, then a stream synchronise
    side = torch.cuda.Stream()
    words = M.words(group, want_pts)
    out, dst = fresh()
    dbytes = torch.full((n, M.SIZE[group]), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    amd.decompress_points(group, ddata, out=out, status=dst, count=False, stream=side, is_async=True)
    amd.compress_points(group, out, out=dbytes, stream=side, is_async=True)
    side.synchronize()
    assert np.array_equal(amd.to_numpy_u64(out), words) and np.array_equal(dst.cpu().numpy(), want_st)
    assert np.array_equal(dbytes.cpu().numpy(), amd.compress_points(group, words))
    # is_async with a count: the count is a host output, so the call has finished on return
    out, dst = fresh()
    _, _, cnt = amd.decompress_points(group, ddata, out=out, status=dst, stream=side, is_async=True)
    assert cnt == bad
    side.synchronize()
    assert np.array_equal(amd.to_numpy_u64(out), words) and np.array_equal(dst.cpu().numpy(), want_st)
    amd.release_stream(side)


@pytest.mark.parametrize("group", GROUPS)
def test_argument_errors(amd, group):
    import torch
    L = amd.lib()
    dec = getattr(L, f"mbls_{group}_decompress")
    com = getattr(L, f"mbls_{group}_compress")
    host, dev = amd.vec_config(), amd.vec_config(is_a_on_device=True, is_result_on_device=True)
    recs = M.to_array(group, list(_member_records(group)[:4]))
    size, nl = M.SIZE[group], NL[group]
    want = M.words(group, _model(group, [bytes(r) for r in recs])[1])
    pts = np.full((4, nl), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    status = np.full(4, 0xAA, dtype=np.uint8)
    cnt = ctypes.c_uint64(0xDEADBEEF)
    out_bytes = np.full((4, size), 0xAA, dtype=np.uint8)
    # device buffers with room for views that start 1 and 8 bytes past a 16-byte boundary
    draw = torch.zeros(4 * size + 16, dtype=torch.uint8, device="cuda")
    draw[:4 * size] = _dev(recs).reshape(-1)
    dpts = torch.full((4 * nl * 8 + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    dstat = torch.full((4,), 0xAA, dtype=torch.uint8, device="cuda")
    assert draw.data_ptr() % 16 == 0 and dpts.data_ptr() % 16 == 0

    def d(b=recs, n=4, c=host, p=pts, st=status, k=cnt):
        return dec(amd._p(b), n, True, ctypes.byref(c) if c is not None else None, amd._p(p), amd._p(st),
                   ctypes.byref(k) if k is not None else None)

    def c_(p=want, n=4, c=host, b=out_bytes):
        return com(amd._p(p), n, True, ctypes.byref(c) if c is not None else None, amd._p(b))

    E = amd.INVALID_ARGUMENT
    assert d(b=None) == E and d(c=None) == E and d(p=None) == E
    assert d(n=0) == E and d(n=-1) == E and d(n=(1 << 26) + 1) == E
    for off in (1, 8):  # a device view that is not 16-byte aligned: the bytes, then the points
        assert d(b=draw[off:], c=dev, p=dpts, st=dstat) == E
        assert d(b=draw, c=dev, p=dpts[off:], st=dstat) == E
    assert c_(p=None) == E and c_(c=None) == E and c_(b=None) == E
    assert c_(n=0) == E and c_(n=-1) == E and c_(n=(1 << 26) + 1) == E
    for off in (1, 8):
        assert c_(p=dpts[off:], c=dev, b=draw) == E
        assert c_(p=dpts, c=dev, b=draw[off:]) == E
    torch.cuda.synchronize()
    # every output stays untouched
    assert (pts == 0xAAAAAAAAAAAAAAAA).all() and (status == 0xAA).all() and cnt.value == 0xDEADBEEF
    assert (out_bytes == 0xAA).all() and bool((dpts == 0xAA).all()) and bool((dstat == 0xAA).all())
    assert np.array_equal(draw[:4 * size].cpu().numpy().reshape(4, size), recs)
    # good calls afterwards: host, then the same device buffers (both outputs may be absent)
    assert d() == amd.SUCCESS
    assert np.array_equal(pts, want) and (status == M.OK).all() and cnt.value == 0
    assert c_() == amd.SUCCESS and np.array_equal(out_bytes, recs)
    assert d(b=draw, c=dev, p=dpts, st=None, k=None) == amd.SUCCESS
    torch.cuda.synchronize()
    assert np.array_equal(dpts[:4 * nl * 8].cpu().numpy().view(np.uint64).reshape(4, nl), want)
    assert bool((dstat == 0xAA).all())
