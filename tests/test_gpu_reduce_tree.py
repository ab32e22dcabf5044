"""G1's level-1 reduction tree (k_reduce_tree8_r28x: levels 0 and 1 of the bucket reduction in one
launch, level 1 as a tree of lane-arithmetic XYZZ additions over eight lanes per segment).

Host tests pin tests/reduce_tree_model.py: the plan it stands on, that its schedule computes the
level's linear forms, its census of (site, class) cells and that a mutant of the group law at a
claimed cell changes the table's final multiple.  Device tests (marked gpu) run the designed tables
and the parity cases of the issue; everything is bit-exact against the oracle, no tolerance.

The reduction plan depends on c and the window count, not on n, so every case here runs the tree:
c = 16 gives level 0 in lanes (8192 segments of 4 per window) and level 1 in 1024 segments of 8."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import msm_reduce_model as M
import reduce_tree_model as T
from helpers import pyref as pr

PKG = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd")
LIB = os.path.join(PKG, "lib", "libbls12_381_mi355x.so")
PLAN = T.plan(*T.KEY)
TABLES = T.tables(PLAN)


class Multiples:
    """k G for signed k as Montgomery rows, built once"""

    def __init__(self):
        self.pts, self.rows = {}, {}

    def point(self, k):
        k %= pr.R
        m = min(k, pr.R - k)
        if m not in self.pts:
            self.pts[m] = pr.g1_mul(m, pr.G1)
        return self.pts[m] if m == k else pr.g1_neg(self.pts[m])

    def row(self, k):
        if k not in self.rows:
            self.rows[k] = np.array(H.g1_affine_mont(self.point(k)), dtype=np.uint64)
        return self.rows[k]


MULT = Multiples()


# ----------------------------------------------------------------------------- host: the model
@pytest.fixture(scope="module")
def lib_host():
    """the binding for host-only calls (msm_plan, msm_reduce_plan)"""
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", PKG, "-j8", "-s"])
    sys.path.insert(0, PKG)
    import bls12_381_amd
    return bls12_381_amd


def test_plan_has_the_tree_level(lib_host):
    lv = PLAN["levels"]
    assert [x["kind"] for x in lv] == ["r28x", "tree8", "wave", "wave", "tree4", "tree4", "tree4"]
    # and these are the kernels the library launches for the unsplit plan, at every size used here
    for n in (1, 64, 1 << 16, *(len(t.entries()) for t in TABLES)):
        sched = lib_host.msm_reduce_plan("g1", n, c=T.KEY[1], bitsize=T.KEY[2])
        assert T.library_levels(sched) == T.model_levels(PLAN), n
        assert [x["launch"] for x in sched["levels"]] == [0, 0, 1, 2, 3, 4, 5]
    assert (lv[1]["m_in"], lv[1]["m_out"], lv[1]["seg_log"], lv[1]["off"], lv[1]["span"]) == (8192, 1024, 3, 0, 4)
    assert PLAN["Wg"] == 9
    # the level count is msm_reduce_model's (the library's: test_gpu_msm_exceptional pins it); the
    # plans whose row level is level 0 (off = 1) keep the row kernel
    assert len(lv) == len(M.plan(*T.KEY)["levels"])
    assert [x["kind"] for x in T.plan("g1", 13, 128)["levels"]][:2] == ["row1", "wave"]


def test_tree_computes_the_segment_forms():
    """U' = sum U_j + sum j V_j and V' = 8 sum V_j for random inputs, short segments included; the
    last level drops V'"""
    rnd = np.random.default_rng(7)
    for cnt in (8, 8, 8, 5, 3, 1):
        V = [int(v) for v in rnd.integers(-50, 50, cnt)]
        U = [int(v) for v in rnd.integers(-50, 50, cnt)]
        Vp, Up = T.tree8(T.Sim(), None, 1, [v % pr.R for v in V], [u % pr.R for u in U])
        assert Up == (sum(U) + sum(j * v for j, v in enumerate(V))) % pr.R
        assert Vp == 8 * sum(V) % pr.R
    # and the design algebra agrees with the schedule
    sites, dbls = T.tree_sites(list(T.GEN_S), list(T.GEN_A))
    assert sum(sites["U'"]) == sum(T.GEN_A) + sum(j * v for j, v in enumerate(T.GEN_S))
    assert dbls["8SV"] * 2 == 8 * sum(T.GEN_S)
    assert set(T.classify(T.GEN_S, T.GEN_A).values()) == {"generic"}


def test_templates_reach_their_cells():
    for (site, cls), (s, a) in T.templates().items():
        assert T.classify(s, a)[site] == cls, (site, cls)


def _census():
    tot, claimed = {}, {}
    for t in TABLES:
        for k, v in t.census.items():
            if k[0] == "tree8":
                tot[k[2:]] = tot.get(k[2:], 0) + v
        for k in t.claims():
            claimed[k[2:]] = claimed.get(k[2:], 0) + 1
    return tot, claimed


# (site, class) cells no input can reach, with the reason; none: every site's operands are
# independent linear forms of the sixteen inputs, and V_j = 4 (bucket sum) takes every value mod r
UNREACHABLE = {}


def test_census_reaches_every_cell():
    tot, claimed = _census()
    missing = []
    for site in T.ADD_SITES:
        for cls in T.ADD_CLASSES:
            have = claimed.get((site, cls), 0) if cls in ("equal", "opposite") else tot.get((site, cls), 0)
            if (site, cls) not in UNREACHABLE and not have:
                missing.append((site, cls))
    for site in T.DBL_SITES:
        if not claimed.get((site, "inf"), 0) or not tot.get((site, "generic"), 0):
            missing.append((site, "inf"))
    assert not missing, missing
    assert not [c for c in UNREACHABLE if tot.get(c)]


@pytest.mark.parametrize("i", range(len(TABLES)), ids=lambda i: TABLES[i].name)
def test_mutants_change_every_claimed_cell(i):
    """equal -> identity, opposite -> doubled, the identity-doubling guard dropped: each must end at
    another multiple of G in every table that claims the cell"""
    t = TABLES[i]
    vacuous = [cell for cell in t.claims() if t.mutated(cell, T.FAULT[cell[3]]) == t.result]
    assert not vacuous, (t.name, vacuous)
    assert set(t.steered) <= set(t.claims()) | {k for k in t.steered if k[3] in ("x_inf", "y_inf")}, t.name


def test_named_tables():
    by = {t.name.split("tree8-")[1]: t for t in TABLES}
    cs = by["wave"].census
    assert cs[("tree8", 1, "W", "equal")] == 8 and cs[("tree8", 1, "U'", "opposite")] == 8
    G = [T.window_sum(PLAN, b)[0] for b in by["window-identity"].m]
    assert G[2] == 0 and by["window-identity"].m[2] and G[1] != 0 and by["window-identity"].result != 0
    assert by["tail"].census[("tree8", 1, "P2", "y_inf")] and by["tail"].result != 0
    for t in TABLES:
        n = len(t.entries())
        assert 1 <= n <= 16384, (t.name, n)
    assert len({abs(k) for t in TABLES for k, _ in t.entries()}) <= 2500


# ----------------------------------------------------------------------------- device
@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gpu_helpers
    gpu_helpers.amd.lib()
    return gpu_helpers.amd


@pytest.fixture(scope="module")
def gh():
    import gpu_helpers
    return gpu_helpers


PLANS = {"glv": dict(c=16), "unsplit": dict(c=16, bitsize=128)}


def _scalars(n, seed, bits):
    s = np.zeros((n, 4), dtype=np.uint64)
    H.oracle().orc_gen_scalars(H.ptr(s), seed, n)
    if bits < 256:  # the unsplit plan's scalars fit its bit size
        s[:, bits // 64:] = 0
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 1 << 16])
@pytest.mark.parametrize("which", list(PLANS))
def test_parity_against_oracle(amd, gh, which, n):
    """n = 1 and 64: almost every tree input is the identity; 2^16 seeded scalars: every bucket
    occupied, the generic path everywhere"""
    cfg = PLANS[which]
    p = amd.msm_plan("g1", n, **cfg)
    assert (p["c"], p["split"], p["Wg"]) == ((16, 2, 8) if which == "glv" else (16, 1, 9)), p
    assert p["levels"] == len(PLAN["levels"])
    s = _scalars(n, 0x5EED0700 + n, 256 if which == "glv" else 128)
    b = np.zeros((n, 12), dtype=np.uint64)
    H.oracle().orc_gen_g1_bases(H.ptr(b), 0x5EED0710 + n, n, 0)
    want = H.g1_from_affine_mont(H.oracle_msm("g1", s, b, fast=n > 8192))
    r = amd.msm("g1", s, b, **cfg)
    assert gh.decode_icicle("g1", r[0]) == want


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(TABLES)), ids=lambda i: TABLES[i].name)
def test_designed_table_on_device(amd, gh, i):
    t = TABLES[i]
    ent = t.entries()
    scal = H.ints_to_limbs([s for _, s in ent], 4)
    bases = np.ascontiguousarray(np.stack([MULT.row(k) for k, _ in ent]))
    want = MULT.point(t.result) if t.result else None
    assert H.g1_from_affine_mont(H.oracle_msm("g1", scal, bases)) == want, f"{t.name}: the oracle and the model disagree"
    assert amd.msm_plan("g1", len(ent), c=16, bitsize=128)["split"] == 1
    r = amd.msm("g1", scal, bases, c=16, bitsize=128)
    assert gh.decode_icicle("g1", r[0]) == want, t.name
    out = amd.msm("g1", scal, bases, icicle=False, c=16, bitsize=128)
    assert gh.decode_jacobian_mont("g1", out[0]) == want, t.name
