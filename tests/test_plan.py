"""CPU-only checks of the MSM schedule the library picks (make_plan through the host-only
mbls_msm_plan diagnostics export; no device work): the split plans and their windows, prepared
tables, and which precompute factors run the shift plan or the split plan on slot 0 of the table
("Shift tables: which plan" and "Window sizes below 2^20"), and the bucket
reduction's kernel schedule (plan_levels through mbls_msm_reduce_plan) against the host model of
tests/reduce_tree_model.py over every plan a caller can reach.  The results of every plan are
checked against the oracle by tests/test_gpu_prepared.py on the GPU."""
import os
import subprocess
import sys

import pytest

import helpers as H

PKG = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd")
LIB = os.path.join(PKG, "lib", "libbls12_381_mi355x.so")


@pytest.fixture(scope="module")
def amd():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", PKG, "-j8", "-s"])
    sys.path.insert(0, PKG)
    import bls12_381_amd
    return bls12_381_amd


@pytest.mark.parametrize("log_n,c", [(8, 8), (13, 8), (14, 11), (15, 11), (16, 16), (20, 16), (24, 16)])
def test_g1_plain_bases_take_the_glv_split(amd, log_n, c):
    p = amd.msm_plan("g1", 1 << log_n)
    assert (p["split"], p["c"], p["F"], p["bstride"], p["prepared"]) == (2, c, 1, 1, 0)
    assert p["W"] == (128 + c - 1) // c
    assert p["buckets"] == p["W"] * (1 << (c - 1))


@pytest.mark.parametrize("log_n,c", [(8, 11), (12, 11), (13, 13), (15, 13), (16, 16), (20, 16)])
def test_g2_plain_bases_take_the_psi_split(amd, log_n, c):
    p = amd.msm_plan("g2", 1 << log_n)
    assert (p["split"], p["c"], p["W"]) == (4, c, (64 + c - 1) // c)


def test_narrow_scalars_and_large_windows_stay_unsplit(amd):
    assert amd.msm_plan("g1", 1 << 16, bitsize=128)["split"] == 1
    assert amd.msm_plan("g2", 1 << 16, bitsize=192)["split"] == 1
    assert amd.msm_plan("g2", 1 << 16, c=18)["split"] == 1  # psi digits need c <= 16
    # a caller's c that leaves the split's top window nearly empty becomes 16
    assert amd.msm_plan("g1", 1 << 20, c=15)["c"] == 16
    assert amd.msm_plan("g1", 1 << 20, c=13)["c"] == 13


@pytest.mark.parametrize("group,F", [("g1", 2), ("g2", 4)])
def test_prepared_tables_take_the_split(amd, group, F):
    for log_n in (8, 16, 20):
        for bits in (0, 64):
            p = amd.msm_plan(group, 1 << log_n, precompute_factor=F, bitsize=bits)
            assert (p["prepared"], p["split"], p["F"], p["bstride"]) == (1, F, 1, 1)
    assert amd.msm_plan("g2", 1 << 16, precompute_factor=4, c=18)["c"] == 16


@pytest.mark.parametrize("F,log_n,c", [(4, 8, 8), (4, 12, 11), (4, 14, 13), (4, 16, 16), (4, 20, 16), (4, 21, 16),
                                       (8, 10, 11), (8, 13, 11), (8, 14, 16), (8, 20, 16),
                                       (16, 8, 8), (16, 10, 16), (16, 19, 16)])
def test_g1_shift_plans_and_windows(amd, F, log_n, c):
    p = amd.msm_plan("g1", 1 << log_n, precompute_factor=F)
    sF = (256 + F - 1) // F
    assert (p["split"], p["F"], p["sF"], p["c"], p["bstride"]) == (1, F, sF, c, 1)
    assert p["Wg"] == (sF + c - 1) // c and p["W"] == F * p["Wg"]


@pytest.mark.parametrize("F,log_n", [(4, 22), (8, 21), (16, 20), (16, 24)])
def test_g1_shift_tables_above_1gib_run_slot0(amd, F, log_n):
    assert (1 << log_n) * F * 96 > 1 << 30
    p = amd.msm_plan("g1", 1 << log_n, precompute_factor=F)
    assert (p["split"], p["bstride"], p["F"], p["c"]) == (2, F, 1, 16)


@pytest.mark.parametrize("group,F", [("g1", 3), ("g1", 5), ("g1", 6), ("g1", 7), ("g1", 32), ("g1", 64),
                                     ("g2", 2), ("g2", 3), ("g2", 5), ("g2", 32)])
def test_other_factors_run_the_split_plan_on_slot0(amd, group, F):
    S = 2 if group == "g1" else 4
    for log_n in (8, 14, 20):
        p = amd.msm_plan(group, 1 << log_n, precompute_factor=F)
        assert (p["split"], p["bstride"], p["F"], p["prepared"]) == (S, F, 1, 0)
        assert p["c"] == amd.msm_plan(group, 1 << log_n)["c"]  # the plain split's window


@pytest.mark.parametrize("F,log_n,c", [(8, 12, 11), (8, 14, 11), (8, 15, 16), (8, 20, 16), (16, 8, 8),
                                       (16, 14, 16)])
def test_g2_shift_plans(amd, F, log_n, c):
    p = amd.msm_plan("g2", 1 << log_n, precompute_factor=F)
    assert (p["split"], p["F"], p["c"], p["bstride"]) == (1, F, c, 1)


def test_plan_argument_errors(amd):
    with pytest.raises(amd.IcicleError):
        amd.msm_plan("g1", 1 << 10, precompute_factor=65)
    with pytest.raises(amd.IcicleError):
        amd.msm_plan("g1", 1 << 10, c=21)
    with pytest.raises(amd.IcicleError):
        amd.msm_plan("g1", 1 << 10, bitsize=257)


# ---- the bucket reduction's kernel schedule (plan_levels through mbls_msm_reduce_plan) -----------
GRID_C = range(2, 21)
GRID_BITS = (1, 32, 64, 127, 128, 129, 192, 193, 255)
GRID_F = (1, 2, 4, 8, 16)
GRID_N = (1, 1 << 12, 1 << 20)
_MODEL = {}


def _grid(amd, group, c):
    for bits in GRID_BITS:
        for F in GRID_F:
            for n in GRID_N:
                cfg = dict(c=c, bitsize=bits, precompute_factor=F)
                yield (n, cfg), amd.msm_plan(group, n, **cfg), amd.msm_reduce_plan(group, n, **cfg)


def _model(group, c, Wg):
    import reduce_tree_model as T
    if (group, c, Wg) not in _MODEL:
        _MODEL[(group, c, Wg)] = T.model_levels(T.plan(group, c, c * Wg - 1))
    return _MODEL[(group, c, Wg)]


@pytest.mark.parametrize("c", GRID_C)
@pytest.mark.parametrize("group", ["g1", "g2"])
def test_reduce_schedule_equals_the_model(amd, group, c):
    """per level the kernel's kind, the segment log and the inputs per window the library launches
    are the ones tests/reduce_tree_model.py plans for the library's own (c, Wg): every caller's c,
    bit sizes around the split thresholds, every kind of table, three sizes"""
    import reduce_tree_model as T
    for case, p, sched in _grid(amd, group, c):
        assert p["levels"] == len(sched["levels"]), (case, p)
        assert T.library_levels(sched) == _model(group, p["c"], p["Wg"]), (case, p)


@pytest.mark.parametrize("c", GRID_C)
@pytest.mark.parametrize("group", ["g1", "g2"])
def test_reduce_schedule_structure(amd, group, c):
    jac, xyzz = (144, 224) if group == "g1" else (288, 448)
    for case, p, sched in _grid(amd, group, c):
        lv = sched["levels"]
        outs = [(x["m_in"] + (1 << x["seg_log"]) - 1) >> x["seg_log"] for x in lv]
        assert lv[0]["m_in"] == 1 << (p["c"] - 1) and outs[-1] == 1, (case, lv)
        for a, o, b in zip(lv, outs, lv[1:]):
            assert b["m_in"] == o and b["raw_in"] == a["raw_out"], (case, lv)
        for x in lv:
            assert x["raw_in"] == (x["kernel"] in ("r28x", "tree8", "r28px")), (case, lv)
            assert not x["raw_out"] or x["kernel"] in ("tree8", "r28px"), (case, lv)
        assert not lv[-1]["raw_out"], (case, lv)
        # launches: one level each, in order, but the tree: exactly levels 0 and 1 of a G1 plan
        tree = [l for l, x in enumerate(lv) if x["kernel"] == "tree8"]
        assert tree in ([], [0, 1]) and (not tree or group == "g1"), (case, lv)
        assert [x["launch"] for x in lv] == [max(l - 1, 0) if tree else l for l in range(len(lv))], (case, lv)
        assert all(x["kernel"] != "r28x" or (l == 0 and group == "g1") for l, x in enumerate(lv)), (case, lv)
        assert all(x["kernel"] != "r28px" or (x["mode"] == "lane" and group == "g2") for x in lv), (case, lv)
        assert sched["bucket_raw"] == lv[0]["raw_in"], (case, sched)
        stored_raw = any(x["raw_out"] and x["kernel"] != "tree8" for x in lv)  # the tree's stay in the lanes
        assert sched["level_bytes"] == (xyzz if stored_raw else jac), (case, sched)


def test_split_plans_stay_on_the_partitioned_sort(amd):
    """a split plan never has c > 16: the GLV / psi digit sources and the per-call image tables
    exist only on the partitioned sort (msm_front), and make_plan rejects a plan that would leave it"""
    for group in ("g1", "g2"):
        for c in GRID_C:
            for case, p, _ in _grid(amd, group, c):
                assert p["split"] == 1 or p["c"] <= 16, (group, case, p)


def test_reduce_schedule_grid_reaches_every_kind(amd):
    import reduce_tree_model as T
    seen = set()
    for group in ("g1", "g2"):
        for c in GRID_C:
            for _, _, sched in _grid(amd, group, c):
                seen |= {k for k, _, _ in T.library_levels(sched)}
    assert seen == {"r28x", "tree8", "r28px", "r28pxU", "row1", "rowU", "wave", "tree4"}


def test_reduce_plan_argument_errors(amd):
    import ctypes
    with pytest.raises(amd.IcicleError):
        amd.msm_reduce_plan("g1", 1 << 10, c=21)
    with pytest.raises(amd.IcicleError):
        amd.msm_reduce_plan("g1", 1 << 10, bitsize=257)
    cfg, out, cnt = amd.msm_config(), (ctypes.c_int32 * 4)(), ctypes.c_int32(0)
    assert amd.lib().mbls_msm_reduce_plan(1, 1 << 20, ctypes.byref(cfg), out, 4, ctypes.byref(cnt)) == 11
    assert cnt.value == 2 + 7 * amd.msm_plan("g1", 1 << 20)["levels"] and list(out) == [0] * 4
    assert amd.lib().mbls_msm_reduce_plan(3, 1 << 20, ctypes.byref(cfg), out, 4, ctypes.byref(cnt)) == 11
    assert amd.lib().mbls_msm_reduce_plan(1, 1 << 20, None, out, 4, ctypes.byref(cnt)) == 3
