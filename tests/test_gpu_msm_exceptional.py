"""The MSM's point additions at their exceptional inputs, where they run: inside the bucket-sum,
reduction and fold chains, beside lanes / pairs / rows that take the generic path.

Every addition after the sort has three data-dependent side branches (an identity operand, equal
operands, opposite operands).  tests/test_gpu_limbs.py pins the formulas one call at a time; this
module steers whole MSMs into them.  Bit-exact everywhere, against pyref (big integers) and the
oracle; no tolerance is involved.

Designed tables (tests/msm_reduce_model.py).  Bases are small signed multiples k G of the
generator and every scalar is (d + 1) 2^(c w), so on the unsplit plans (G1 bitsize 128, G2
bitsize 192) entry i lands in bucket d of window w and nowhere else.  The model replays the
reduction levels and the fold over integers mod r and counts, per (kernel kind, level, phase),
how often an addition is generic / x_inf / y_inf / equal / opposite.  The CPU tests here pin the
model's plan and digits to the library, require every reachable (kind, phase, class) cell from
the tables together, and require that a mutant of the group law at a claimed cell changes the
table's final multiple (a wrong intermediate that is later cancelled or weighted 0 would be a
vacuous claim).  The device tests then run every table through k_final_icicle (result on the
device) and through the raw entry's k_final.

Heavy buckets with related points (default split plans).  All scalars equal, bases all P / half
P half -P / cycling P, 2P, -3P: every node of the heavy-slice adders (XYZZ strided chains, the
lane tree, wave_sum16, row_tree and the group sums) adds equal, opposite or closely related
operands.  The sums are order-independent, so the expected values are closed forms; NO census is
claimed here: the model does not cover the slice plan and the order inside a bucket is the
sort's business.

Accumulation, mid-chunk.  The order inside a bucket is not promised, so only multisets whose
every order passes a branch are used, all drawn from {P, -P} (every pair of elements shares x):
  {P, P, P, P}     the chunk's second step is P + P (doubling) in every order; then 2P + P, 3P + P.
  {P, P, -P, -P}   the second step is a doubling (P, P / -P, -P first) or a cancellation (mixed);
                   the partial sum before the last step is +-P and the last element its
                   opposite, so the last step (xmadd, in mid-chunk) cancels in every order; after
                   a cancellation at step 2 the chain restarts from the identity.
  {P, P, P, -P}    the second step doubles or cancels in every order; the sum is 2P.
  {P, -P, -P}      likewise; the sum is -P.
{P, P, -P, -P, Q} is run too (most orders pass a branch, orders that open with Q and P do not):
its expected value holds for every order, it carries no per-order claim.  Each multiset fills 96
buckets with the index order inside the bucket rotated from bucket to bucket.

G2 pair votes.  The pair-sliced predicates decide "PP == 0" by a vote of the two lanes
(r28p::is_zero_lt2p -> both).  Pairs of points of E' whose x difference has exactly one zero Fq2
component, or equal / opposite components -- (d, 0), (0, d), (d, d), (d, -d) -- separate "both
lanes vote" from "each lane decides": for Pd = (0, d) PP = (-d^2, 0), for (d, d) PP = (0, 2 d^2).
On the unsplit plan the bases need only lie on E' (no endomorphism is applied), so the pairs are
built by square roots in Fq2.  Each pair is placed as a chunk's first two points (xmmadd), after
a cancelling pair T, -T in a chunk (xmadd from a restarted accumulator, if the sort keeps the
index order), in adjacent buckets of one level-0 lane segment (r28px::xadd as R and V_t, both
records at zz = 1) and as the two U records of one level-1 lane segment (r28px::xadd as S and
U_t: buckets {A, -A} and {B, -B} make the level-0 outputs U' = A, B with V' the identity; a
level-1 V is a doubled sum, so no pure pair reaches R += V_t there).  The expected values come
from pyref.msm; test_oracle_agrees_off_subgroup shows once that the oracle agrees with it on
such points."""
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import helpers as H
import msm_reduce_model as M
import reduce_tree_model as T
from helpers import pyref as pr

PKG = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd")
LIB = os.path.join(PKG, "lib", "libbls12_381_mi355x.so")


# ----------------------------------------------------------------------------- shared, built once
class Multiples:
    """k G for signed k, affine (pyref) and as Montgomery rows; built once per module"""

    def __init__(self, group):
        self.group = group
        self.base = pr.G1 if group == "g1" else pr.G2
        self.mul = pr.g1_mul if group == "g1" else pr.g2_mul
        self.neg = pr.g1_neg if group == "g1" else pr.g2_neg
        self.enc = H.g1_affine_mont if group == "g1" else H.g2_affine_mont
        self.pts, self.rows = {}, {}

    def point(self, k):
        k %= pr.R
        m = min(k, pr.R - k)
        if m not in self.pts:
            self.pts[m] = self.mul(m, self.base)
        return self.pts[m] if m == k else self.neg(self.pts[m])

    def row(self, k):
        if k not in self.rows:
            self.rows[k] = np.array(self.enc(self.point(k)), dtype=np.uint64)
        return self.rows[k]

    def arrays(self, entries):
        """[(signed multiple, scalar)] -> (scalars (n, 4), bases (n, 12 | 24)) u64"""
        scal = H.ints_to_limbs([s for _, s in entries], 4)
        bases = np.ascontiguousarray(np.stack([self.row(k) for k, _ in entries]))
        return scal, bases


MULT = {"g1": Multiples("g1"), "g2": Multiples("g2")}
TABLES = M.all_tables()
TABLE_IDS = [(key, i) for key, ts in TABLES.items() for i in range(len(ts))]


def _tid(p):
    key, i = p
    return TABLES[key][i].name


def from_mont(group, row):
    return H.g1_from_affine_mont(row) if group == "g1" else H.g2_from_affine_mont(row)


@pytest.fixture(scope="module")
def lib_host():
    """the binding for host-only calls (msm_plan)"""
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", PKG, "-j8", "-s"])
    sys.path.insert(0, PKG)
    import bls12_381_amd
    return bls12_381_amd


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


# ----------------------------------------------------------------------------- CPU: plan, digits
EXPECTED_KINDS = {
    ("g1", 5, 128): ["wave", "tree4"],
    ("g1", 13, 128): ["row1", "wave", "tree4", "tree4", "tree4", "tree4"],
    ("g1", 16, 128): ["r28x", "rowU", "wave", "wave", "tree4", "tree4", "tree4"],
    ("g2", 5, 192): ["wave", "tree4"],
    ("g2", 16, 192): ["r28px", "r28pxU", "r28pxU", "wave", "wave", "tree4", "tree4", "tree4", "tree4"],
    ("g2", 18, 192): ["r28px", "r28pxU", "r28pxU", "rowU", "wave", "wave", "tree4", "tree4", "tree4"],
}


@pytest.mark.parametrize("key", M.PLANS, ids=lambda k: f"{k[0]}-c{k[1]}")
def test_model_plan_matches_library(lib_host, key):
    """the model's restatement of make_plan / plan_levels against mbls_msm_plan: unsplit, the
    caller's c, W = Wg = ceil((bitsize + 1) / c), the same number of levels -- at every n the
    tables use (the plan depends on c and Wg, not on n)"""
    group, c, bits = key
    pl = M.plan(*key)
    sizes = {len(t.entries()) for t in TABLES[key]} | {1, 4096}
    for n in sorted(sizes):
        p = lib_host.msm_plan(group, n, c=c, bitsize=bits)
        assert (p["split"], p["c"], p["W"], p["Wg"], p["F"]) == (1, c, pl["W"], pl["Wg"], 1), (n, p)
        assert p["buckets"] == pl["Wg"] * pl["B"]
        assert p["levels"] == len(pl["levels"]), (n, p)
        # the kernels msm_device launches, from the library itself (level 1 of ("g1", 16, 128) is
        # the tree since reduce_tree_model; this module's tables keep the chain's census there)
        assert T.library_levels(lib_host.msm_reduce_plan(group, n, c=c, bitsize=bits)) == \
            T.model_levels(T.plan(*key)), (n, p)
    assert [lv["kind"] for lv in pl["levels"]] == EXPECTED_KINDS[key]
    # the shapes the designs lean on: a short last tree segment, a row level at off = 1, lane
    # levels with U and 2-input segments
    lv = pl["levels"]
    assert lv[0]["off"] == 1 and all(x["off"] == 0 and x["has_u"] for x in lv[1:]) and not lv[0]["has_u"]
    assert lv[-1]["m_out"] == 1 and lv[-1]["last"]
    for a, b in zip(lv, lv[1:]):
        assert b["m_in"] == a["m_out"] and b["span"] == a["span"] << a["seg_log"]
    if key in (("g1", 13, 128), ("g2", 16, 192)):
        assert lv[-1]["kind"] == "tree4" and lv[-1]["m_in"] == 2  # cnt < 4
    if group == "g2" and c >= 16:
        assert [x["seg_log"] for x in lv[:3]] == [2, 1, 1]


@pytest.mark.parametrize("key", M.PLANS, ids=lambda k: f"{k[0]}-c{k[1]}")
def test_digits_land_where_designed(key):
    """pyref.signed_digits of every designed scalar: one digit, d + 1, in window w, no carry
    (bucket d carries weight d + 1 at level 0); the largest digit 2^(c-1) stays positive and
    lands in the top bucket"""
    group, c, bits = key
    pl = M.plan(*key)
    for t in TABLES[key]:
        where = [(w, d) for w, b in enumerate(t.m) for d in sorted(b)]
        ent = t.entries()
        assert len(ent) == len(where)
        for (k, s), (w, d) in zip(ent, where):
            assert k == t.m[w][d] and k != 0 and s < (1 << bits)
            digits, carry = pr.signed_digits(s, c, pl["W"])
            assert carry == 0 and digits == [d + 1 if j == w else 0 for j in range(pl["W"])], (t.name, w, d)
    half = 1 << (c - 1)
    for w in (0, 1, pl["W"] - 2):
        digits, carry = pr.signed_digits(half << (c * w), c, pl["W"])
        assert carry == 0 and digits[w] == half and sum(1 for d in digits if d) == 1
        assert digits[w] - 1 == pl["B"] - 1  # the top bucket
    digits, carry = pr.signed_digits((half + 1) << c, c, pl["W"])  # one more turns negative and carries
    assert digits[1] == half + 1 - (1 << c) and digits[2] == 1


def test_table_sizes_stay_small():
    """n in the hundreds to low thousands; a few hundred distinct multiples per group"""
    for key, ts in TABLES.items():
        for t in ts:
            assert 1 <= len(t.entries()) <= 4096, (t.name, len(t.entries()))
    for group in ("g1", "g2"):
        ks = {abs(k) for key, ts in TABLES.items() if key[0] == group for t in ts for k, _ in t.entries()}
        assert len(ks) <= 600 and max(ks) < 1 << 40, (group, len(ks))


# ----------------------------------------------------------------------------- CPU: census
CLASSES = ("equal", "opposite", "x_inf", "y_inf")
LANE_GUARD = "the lane kernels never hand an identity operand to the adder (xadd_raw skips identity records, " \
             "S += R is guarded by !R.is_inf()); the guarded S += R onto a live S is counted as class `guard`"


def _unreachable():
    """(kind, phase, class) -> reason.  Everything else in kinds x phases x CLASSES must be reached."""
    u = {}
    for kind in ("r28x", "r28px", "row1"):
        for cls in CLASSES:
            u[(kind, "S+=U", cls)] = "level 0 has no U"
    for kind in M.LANE_KINDS:
        for ph in ("R+=V", "S+=R", "S+=U"):
            u.setdefault((kind, ph, "y_inf"), LANE_GUARD)
        u[(kind, "dbl", "inf")] = "the doublings of R are guarded by !R.is_inf()"
    for cls in ("equal", "opposite", "guard"):
        u[("r28pxU", "S+=R", cls)] = "2-input segments at off = 0: S += R runs only at the top input, where S is " \
                                     "still the identity (the bottom input has weight 0)"
    return u


def _cells():
    cells = []
    for kind in M.KINDS:
        if kind == "fold":
            phases = ("add",)
        elif kind == "tree4":
            phases = M.TREE_SITES
        else:
            phases = ("R+=V", "S+=R", "S+=U")
        cells += [(kind, ph, cls) for ph in phases for cls in CLASSES]
        cells.append((kind, "dbl", "inf"))
        if kind in M.LANE_KINDS:
            cells.append((kind, "S+=R", "guard"))
    return cells


def _census():
    """(whole census, claimed census) over all tables, keyed (kind, phase, class).  equal /
    opposite / guard count only where a table claims them (the level it aims at: there the
    mutant test holds it answerable); identity operands count wherever they occur"""
    tot, claimed = Counter(), Counter()
    for ts in TABLES.values():
        for t in ts:
            for (kind, _, ph, cls), v in t.census.items():
                tot[(kind, ph, cls)] += v
            for kind, _, ph, cls in t.claims():
                claimed[(kind, ph, cls)] += 1
    return tot, claimed


def _census_text(tot, claimed):
    rows = []
    for kind, ph in sorted({k[:2] for k in tot}):
        cl = {k[2]: v for k, v in tot.items() if k[:2] == (kind, ph)}
        cm = {k[2]: v for k, v in claimed.items() if k[:2] == (kind, ph)}
        rows.append(f"{kind:7s} {ph:5s} " + " ".join(f"{c}={cl[c]}" for c in sorted(cl)) + "   claimed by tables: " +
                    " ".join(f"{c}={cm[c]}" for c in sorted(cm)))
    return "\n".join(rows)


def test_census_reaches_every_reachable_cell():
    tot, claimed = _census()
    unreachable = _unreachable()
    text = _census_text(tot, claimed)
    missing, ghosts = [], []
    for cell in _cells():
        count = claimed[cell] if cell[2] in ("equal", "opposite", "guard") else tot[cell]
        if cell in unreachable:
            if tot[cell]:
                ghosts.append((cell, unreachable[cell]))
        elif count < 1:
            missing.append(cell)
    assert not ghosts, f"cells listed as unreachable were reached: {ghosts}\n{text}"
    assert not missing, f"cells no designed table reaches: {missing}\n{text}"
    # every kernel kind of the issue is there, and the chains see generic neighbours too
    for kind in M.KINDS:
        assert any(k[0] == kind and k[2] == "generic" and v for k, v in tot.items()), kind


def test_families_reach_what_they_are_named_for():
    """the named families, at the place they aim at (per table, not only in the sum)"""
    for key, ts in TABLES.items():
        pl = M.plan(*key)
        by = {t.name: t for t in ts}
        pre = f"{key[0]}-c{key[1]}-"
        for lvl, lv in enumerate(pl["levels"]):
            if lv["kind"] == "tree4":
                continue
            cs = by[f"{pre}L{lvl}-{lv['kind']}"].census
            k = (lv["kind"], lvl)
            assert cs[k + ("R+=V", "equal")] and cs[k + ("R+=V", "opposite")], (key, lvl)
            if lv["has_u"]:
                assert cs[k + ("S+=U", "equal")] and cs[k + ("S+=U", "opposite")], (key, lvl)
            if lv["kind"] != "r28pxU":
                assert cs[k + ("S+=R", "equal")] and cs[k + ("S+=R", "opposite")], (key, lvl)
            if lv["kind"] in M.LANE_KINDS:
                if lv["kind"] != "r28pxU":
                    assert cs[k + ("S+=R", "guard")], (key, lvl)  # R the identity in mid-segment, S live
            elif not lv["last"]:
                assert cs[k + ("dbl", "inf")], (key, lvl)  # Vout doubles the identity
        f = by[pre + "fold-equal-opposite"].census
        assert f[("fold", -1, "add", "equal")] == 1 and f[("fold", -1, "add", "opposite")] == 1
        assert f[("fold", -1, "dbl", "inf")] >= 2 * pl["c"]  # the top window and the cancelled accumulator
        assert by[pre + "fold-leading-identity"].census[("fold", -1, "dbl", "inf")] == pl["c"] * (pl["Wg"] - 3)
        assert by[pre + "msm-identity-windows"].result == 0 and by[pre + "msm-identity-fold"].result == 0
        assert by[pre + "msm-identity-fold"].census[("fold", -1, "add", "opposite")] == 1
        assert by[pre + "window-identity"].result != 0 and by[pre + "one-live-window"].result != 0


@pytest.mark.parametrize("p", TABLE_IDS, ids=_tid)
def test_mutants_change_every_claimed_cell(p):
    """a model that mishandles one claimed cell -- equal operands give the identity, opposite
    operands give the doubled point, the lane kernels' !R.is_inf() guard is dropped -- must end
    at another multiple; else the device test could not see that bug through this table"""
    t = TABLES[p[0]][p[1]]
    vacuous = [cell for cell in t.claims() if t.mutated(cell, M.FAULT[cell[3]]) == t.result]
    assert not vacuous, (t.name, vacuous)
    if t.target >= 0:
        assert t.claims(), t.name


def test_mutants_are_wired():
    """the mutation itself: each fault changes the adder's answer at its own cell only"""
    cell = ("wave", 3, "R+=V", "equal")
    assert M.Sim().add(cell[:3], 5, 5) == 10
    assert M.Sim((cell, "equal_inf")).add(cell[:3], 5, 5) == 0
    assert M.Sim((cell, "equal_inf")).add(("wave", 2, "R+=V"), 5, 5) == 10
    opp = ("wave", 3, "R+=V", "opposite")
    assert M.Sim().add(opp[:3], 5, pr.R - 5) == 0 and M.Sim((opp, "opposite_dbl")).add(opp[:3], 5, pr.R - 5) == 10
    g = ("r28x", 0, "S+=R", "guard")
    assert M.Sim().guarded(g[:3], 7) == 7 and M.Sim((g, "guard")).guarded(g[:3], 7) == 0


def test_model_replays_plain_sums():
    """the schedule restatement itself: for random sparse tables the replayed result is
    sum_w 2^(c w) sum_d (d + 1) m[w][d], whatever the kernels' association"""
    rnd = np.random.default_rng(5)
    for key in M.PLANS:
        pl = M.plan(*key)
        t = M.Table("random", pl, -1)
        for _ in range(300):
            w = int(rnd.integers(0, pl["Wg"] - 1))
            d = int(rnd.integers(0, min(pl["B"], 1 << 10)))
            t.put(w, d, int(rnd.integers(-9, 10)))
        want = sum(((d + 1) * v) << (pl["c"] * w) for w, b in enumerate(t.m) for d, v in b.items()) % pr.R
        assert t.result == want, key


# ----------------------------------------------------------------------------- device: the tables
def _run_msm(amd, gh, group, scal, bases, icicle, **cfg):
    """icicle=True: ICICLE entry with the result on the device (k_final_icicle); False: the raw
    entry (k_final, Jacobian Montgomery)"""
    import torch
    n = scal.shape[0]
    ds, db = amd.torch_u64(scal), amd.torch_u64(bases)
    if icicle:
        out = torch.zeros((1, 18 if group == "g1" else 36), dtype=torch.int64, device="cuda")
        amd.msm(group, ds, db, icicle=True, out=out, n=n, **cfg)
        torch.cuda.synchronize()
        return gh.decode_icicle(group, amd.to_numpy_u64(out)[0])
    out = amd.msm(group, ds, db, icicle=False, n=n, **cfg)
    return gh.decode_jacobian_mont(group, out[0])


@pytest.mark.gpu
@pytest.mark.parametrize("p", TABLE_IDS, ids=_tid)
def test_designed_table_on_device(amd, gh, p):
    key, i = p
    group, c, bits = key
    t = TABLES[key][i]
    mult = MULT[group]
    scal, bases = mult.arrays(t.entries())
    want = mult.point(t.result) if t.result else None
    ref = from_mont(group, H.oracle_msm(group, scal, bases))
    assert ref == want, f"{t.name}: the oracle and the model disagree"
    assert amd.msm_plan(group, scal.shape[0], c=c, bitsize=bits)["split"] == 1
    for icicle in (True, False):
        got = _run_msm(amd, gh, group, scal, bases, icicle, c=c, bitsize=bits)
        assert got == want, (t.name, "k_final_icicle" if icicle else "k_final")


# ----------------------------------------------------------------------------- device: heavy buckets
def _heavy_scalar():
    """one scalar whose GLV digits (c = 8, 16) and psi digits (c = 13, 16) are all non-zero"""
    rnd = pr.rng(0xE4CE)
    while True:
        s = pr.random_fr(rnd)
        m1, _, m2, _ = pr.glv_decompose(s)
        ok = all(all(pr.signed_digits(m, c, (128 + c - 1) // c)[0]) for m in (m1, m2) for c in (8, 16))
        ok = ok and all(all(pr.signed_digits(m, c, (64 + c - 1) // c)[0]) for m, _ in pr.psi_decompose(s)
                        for c in (13, 16))
        if ok:
            return s


HEAVY_S = _heavy_scalar()
# With one repeated scalar every window's contributions share one bucket per digit stream: 16
# buckets of n / 16 sixteen-point chunk partials each (the average bucket of these plans has 128, 8, 8
# and 8 contributions, an eighth of which is at most 16, so accumulate_chunk stays 16), all heavy (> SMALL_MAX partials).  The slice length is
# 256 partials while 16 n / 16 partials spread over the 512 slice workgroups stay under 256 each,
# so a bucket has > HEAVY_GROUP = 16 slices -- and group sums -- from 4097 partials: G1 2^17 has 32
# slices per bucket, G2 16 * 4097 the fewest possible, 17.
HEAVY_CASES = [("g1", 8192), ("g1", 1 << 17), ("g2", 8192), ("g2", 16 * 4097)]
HEAVY_PATTERNS = {"all_P": (1,), "half_P_half_minus_P": None, "cycle_P_2P_minus_3P": (1, 2, -3)}


def test_heavy_scalar_digits(lib_host):
    """the split plans these cases run, and that every digit stream of the scalar is non-zero in
    every window (each window's contributions then share one bucket per stream)"""
    for group, n in HEAVY_CASES:
        p = lib_host.msm_plan(group, n)
        assert p["split"] == (2 if group == "g1" else 4)
        mags = [m for m in pr.glv_decompose(HEAVY_S)[0::2]] if group == "g1" else [m for m, _ in pr.psi_decompose(HEAVY_S)]
        for m in mags:
            assert all(pr.signed_digits(m, p["c"], p["W"])[0]), (group, n, p)
        # > 16 partials per bucket: the heavy path; the large cases > 16 slices of 256 partials
        assert n // 16 > 16
    assert (1 << 17) // 16 > 16 * 256 and 4097 > 16 * 256


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", list(HEAVY_PATTERNS))
@pytest.mark.parametrize("group,n", HEAVY_CASES, ids=lambda v: str(v))
def test_heavy_buckets_related_points(amd, gh, group, n, pattern):
    mult = MULT[group]
    if pattern == "half_P_half_minus_P":
        ks = [1] * (n // 2) + [-1] * (n - n // 2)
    else:
        cyc = HEAVY_PATTERNS[pattern]
        ks = [cyc[i % len(cyc)] for i in range(n)]
    uniq = {k: mult.row(k) for k in set(ks)}
    bases = np.ascontiguousarray(np.stack([uniq[k] for k in ks]))
    scal = np.ascontiguousarray(np.tile(H.ints_to_limbs([HEAVY_S], 4), (n, 1)))
    total = sum(ks) * HEAVY_S % pr.R
    want = mult.point(total) if total else None
    if pattern == "half_P_half_minus_P":
        assert want is None
    # the checker's restatement; its window-parallel Pippenger at the sizes where that takes seconds
    assert from_mont(group, H.oracle_msm(group, scal, bases, fast=n > 8192)) == want
    assert _run_msm(amd, gh, group, scal, bases, True) == want
    if n == 8192:
        assert _run_msm(amd, gh, group, scal, bases, False) == want


# ----------------------------------------------------------------------------- device: mid-chunk
MULTISETS = [(1, 1, 1, 1), (1, 1, -1, -1), (1, 1, 1, -1), (1, -1, -1), (1, 1, -1, -1, 5)]
MID_BUCKETS = 96


def _mid_chunk_entries(c):
    """every multiset in MID_BUCKETS buckets of its own window, the order inside the bucket
    rotated (and every other bucket reversed) from bucket to bucket"""
    ent, total = [], 0
    for w, ms in enumerate(MULTISETS):
        for d in range(MID_BUCKETS):
            r = d % len(ms)
            order = list(ms[r:] + ms[:r])
            if (d // len(ms)) % 2:
                order.reverse()
            s = (d + 1) << (c * w)
            ent += [(k, s) for k in order]
            total += sum(ms) * s
    return ent, total % pr.R


def test_mid_chunk_orders_pass_a_branch():
    """the per-order argument of the module docstring, by enumeration: every order of the
    multisets drawn from {P, -P} doubles or cancels at its second step, and the zero-sum one
    cancels at its last step"""
    from itertools import permutations
    for ms in MULTISETS[:4]:
        for order in set(permutations(ms)):
            assert abs(order[0]) == abs(order[1]) == 1
            acc = list(np.cumsum(order))
            if sum(ms) == 0:
                assert abs(acc[-2]) == 1 and order[-1] == -acc[-2]


@pytest.mark.gpu
@pytest.mark.parametrize("group,c,bits", [("g1", 13, 128), ("g1", 16, 128), ("g2", 13, 192), ("g2", 16, 192)])
def test_mid_chunk_exceptional_multisets(amd, gh, group, c, bits):
    mult = MULT[group]
    ent, total = _mid_chunk_entries(c)
    scal, bases = mult.arrays(ent)
    want = mult.point(total)
    assert amd.msm_plan(group, len(ent), c=c, bitsize=bits)["split"] == 1
    assert from_mont(group, H.oracle_msm(group, scal, bases)) == want
    assert _run_msm(amd, gh, group, scal, bases, True, c=c, bitsize=bits) == want
    assert _run_msm(amd, gh, group, scal, bases, False, c=c, bitsize=bits) == want


# ----------------------------------------------------------------------------- G2 pair votes
def _f2_pow(a, e):
    acc = (1, 0)
    while e:
        if e & 1:
            acc = pr.f2_mul(acc, a)
        a = pr.f2_mul(a, a)
        e >>= 1
    return acc


def f2_sqrt(a):
    """a square root of a in Fq2 = Fq[u] / (u^2 + 1), p = 3 mod 4, or None (Adj, Rodriguez-Henriquez
    alg. 9)"""
    if a == (0, 0):
        return (0, 0)
    a1 = _f2_pow(a, (pr.P - 3) // 4)
    alpha = pr.f2_mul(pr.f2_mul(a1, a1), a)
    a0 = pr.f2_mul((alpha[0], (-alpha[1]) % pr.P), alpha)  # alpha^p alpha
    if a0 == (pr.P - 1, 0):
        return None
    x0 = pr.f2_mul(a1, a)
    if alpha == (pr.P - 1, 0):
        r = pr.f2_mul((0, 1), x0)
    else:
        r = pr.f2_mul(_f2_pow(pr.f2_add((1, 0), alpha), (pr.P - 1) // 2), x0)
    return r if pr.f2_mul(r, r) == a else None


def _rhs(x):
    return pr.f2_add(pr.f2_mul(pr.f2_mul(x, x), x), pr.G2_B)


SHAPES = {"(d,0)": lambda d: (d, 0), "(0,d)": lambda d: (0, d), "(d,d)": lambda d: (d, d),
          "(d,-d)": lambda d: (d, pr.P - d)}


def _vote_pairs():
    """{shape: (A, B)} on E' with x_B - x_A of that shape"""
    rnd = pr.rng(0x9A12)
    out = {}
    for name, shape in SHAPES.items():
        while name not in out:
            x1 = (pr.random_fq(rnd), pr.random_fq(rnd))
            d = pr.random_fq(rnd)
            x2 = pr.f2_add(x1, shape(d))
            y1, y2 = f2_sqrt(_rhs(x1)), f2_sqrt(_rhs(x2))
            if d and y1 is not None and y2 is not None:
                out[name] = ((x1, y1), (x2, y2))
    return out


_PAIRS = None


def vote_pairs():
    global _PAIRS
    if _PAIRS is None:
        _PAIRS = _vote_pairs()
    return _PAIRS


VOTE_C, VOTE_BITS = 16, 192


def _vote_entries(A, B, T):
    """[(point, scalar)]: the pair in the four places of the module docstring, each in a window of
    its own and in segments of their own, beside generic neighbours (multiples of T)"""
    c = VOTE_C
    nA, nB, nT = pr.g2_neg(A), pr.g2_neg(B), pr.g2_neg(T)
    ent = []

    def at(w, d, *pts):
        ent.extend((p, (d + 1) << (c * w)) for p in pts)

    for rep in range(4):  # a few buckets each: the order inside a bucket is the sort's
        at(0, 40 + 3 * rep, A, B)                  # a chunk's first two points
        at(0, 41 + 3 * rep, B, A)
        at(1, 40 + 2 * rep, T, nT, A, B)           # after a cancelling pair: xmadd from the identity
    # level 0, window 2: buckets 4 q + 3 and 4 q + 2 of segment q = 5 (R = A, then R += B),
    # segment 4 and 6 generic
    at(2, 23, A)
    at(2, 22, B)
    at(2, 19, T)
    at(2, 18, A)
    at(2, 26, B)
    at(2, 25, T)
    # level 1, window 3: level-1 segment q = 5 reads level-0 segments 11 (top) and 10;
    # buckets {A at weight 2, -A at weight 1} leave U' = A and V' the identity
    at(3, 4 * 11 + 1, A)
    at(3, 4 * 11, nA)
    at(3, 4 * 10 + 1, B)
    at(3, 4 * 10, nB)
    at(3, 4 * 8 + 1, T)
    at(3, 4 * 13, T)
    return ent


def _g2_arrays(ent):
    scal = H.ints_to_limbs([s for _, s in ent], 4)
    bases = np.array([H.g2_affine_mont(p) for p, _ in ent], dtype=np.uint64).reshape(-1, 24)
    return scal, np.ascontiguousarray(bases)


def test_vote_pairs_are_on_the_twist():
    for name, (A, B) in vote_pairs().items():
        assert pr.g2_on_curve(A) and pr.g2_on_curve(B), name
        dx = pr.f2_sub(B[0], A[0])
        assert dx == SHAPES[name](dx[0] if dx[0] else dx[1]) and dx != (0, 0), name
        assert pr.g2_add(pr.g2_mul(pr.R - 1, A), A) is not None  # r A != 0: outside the subgroup
    assert f2_sqrt((pr.P - 1, 0)) in ((0, 1), (0, pr.P - 1)) and f2_sqrt((4, 0)) in ((2, 0), (pr.P - 2, 0))


def test_oracle_agrees_off_subgroup():
    """the oracle's MSM against pyref.msm on points of E' outside G2, small scalars (the group law
    does not care about the subgroup; the digit code must not reduce them differently)"""
    A, B = vote_pairs()["(0,d)"]
    pts = [A, B, pr.g2_neg(A), pr.G2, B]
    sc = [3, (1 << 70) + 5, 1 << 16, 9, (23 << 48) + 1]
    scal, bases = _g2_arrays(list(zip(pts, sc)))
    assert H.g2_from_affine_mont(H.oracle_msm("g2", scal, bases)) == pr.msm(sc, pts, "g2")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_g2_pair_votes(amd, gh, shape):
    A, B = vote_pairs()[shape]
    T = pr.g2_mul(7, pr.G2)
    ent = _vote_entries(A, B, T)
    scal, bases = _g2_arrays(ent)
    assert amd.msm_plan("g2", len(ent), c=VOTE_C, bitsize=VOTE_BITS)["split"] == 1
    # pyref.msm by buckets of equal scalars (the same sum, fewer scalar multiplications)
    by = {}
    for p, s in ent:
        by[s] = pr.g2_add(by.get(s), p)
    want = pr.msm(list(by), list(by.values()), "g2")
    assert H.g2_from_affine_mont(H.oracle_msm("g2", scal, bases)) == want
    assert _run_msm(amd, gh, "g2", scal, bases, True, c=VOTE_C, bitsize=VOTE_BITS) == want
    assert _run_msm(amd, gh, "g2", scal, bases, False, c=VOTE_C, bitsize=VOTE_BITS) == want
