"""CPU-only checks of the MSM front's contract model (tests/front_model.py) and of the cases
tests/test_gpu_front.py runs on the device (tests/front_cases.py): every case's plan is the one it
was designed for (through the host-only mode of mbls_msm_front_probe), the model's digits reproduce
its scalars, the case sits in its cell of the branch census, and the model's own tables pass
check().  Then the checker itself: each mutation of correct tables must make check() fail, at the
table named here -- a checker that passes a mutant is a failure of this file."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import front_cases as fc
import front_model as fm

PKG = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd")
LIB = os.path.join(PKG, "lib", "libbls12_381_mi355x.so")


@pytest.fixture(scope="module")
def amd():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", PKG, "-j8", "-s"])
    sys.path.insert(0, PKG)
    import bls12_381_amd
    return bls12_381_amd


def designed_plan(amd, case):
    """the plan and table capacities of a case, after asserting the fields it pins"""
    info = amd.msm_front_plan(case.group, case.n, **case.cfg)
    got = {k: info["plan"][k] for k in case.plan}
    assert got == case.plan, f"{case.name} no longer runs the plan it was designed for"
    return info["plan"], info["words"]


def test_constants_are_the_sources():
    assert fm.DT_TILE == fm.K["DT_THREADS"] * fm.K["MBLS_DT_PER"] and fm.PS_KEEP == fm.PS_RK * fm.PS_TEAM
    assert fm.FILL == int.from_bytes(b"\xa5" * 4, "little")
    # the cases below are written for these relations; a retune that breaks one must revisit them
    assert fm.PH_MIN > fm.PS_STAGE > fm.PS_KEEP and fm.PH_MIN + 1 > 2 * fm.DT_TILE
    assert fm.HEAVY_SLICE * fm.CHUNK >= fm.PH_MIN


@pytest.mark.parametrize("name", [k.name for k in fc.CASES])
def test_case_reaches_its_cell_and_the_model_checks(amd, name):
    case = fc.BY_NAME[name]
    plan, words = designed_plan(amd, case)
    scalars = case.scalars()
    D = fm.model_digits(plan, scalars)
    want = fm.scalar_ints(scalars) % fm.pr.R
    assert (fm.digit_values(plan, D) == want).all(), "the model's digits do not reproduce the scalars"
    # magnitudes in [1 - B, B]; a split's negative half / quarter flips the range
    assert np.abs(D).max(initial=0) <= plan["B"] and (plan["split"] > 1 or D.min(initial=0) >= 1 - plan["B"])
    z = fm.census(plan, D)
    assert case.cell(z), f"{name} left its census cell: {z}"
    assert case.n <= 1 << 18
    fm.check(fm.model_tables(plan, D, words), plan, scalars, digits=D)


def test_probe_plan_mode_and_arguments(amd):
    """without tables the probe is host only: the plan msm_plan reports, the chunk length of
    accumulate_chunk, capacities that cover every table; and its argument checks"""
    import ctypes
    for group, n, cfg in (("g1", 1 << 20, {}), ("g2", 1 << 16, {}), ("g1", 1 << 24, {}), ("g1", 300, dict(precompute_factor=8))):
        info = amd.msm_front_plan(group, n, **cfg)
        plan, words, mp = info["plan"], info["words"], amd.msm_plan(group, n, **cfg)
        assert all(plan[k] == mp[k] for k in ("c", "W", "Wg", "F", "sF", "split", "prepared", "bstride"))
        assert plan["TB"] == mp["buckets"] == plan["Wg"] * plan["B"] and plan["B"] == 1 << (plan["c"] - 1)
        assert plan["contributions"] == n * plan["W"] * plan["split"]
        assert plan["chunk"] == max(fm.CHUNK, plan["contributions"] // plan["TB"] // 8)
        TB, NC, L = plan["TB"], plan["contributions"], plan["chunk"]
        assert words["sorted"] >= NC and min(words[k] for k in ("offsets", "nchunks", "chunk_off")) >= TB + 3
        assert words["owner"] >= NC // L + TB and words["first"] >= NC // L + 1 and words["perm"] >= TB
        assert words["binbase"] >= fm.order_words(TB) + 1 and words["H_gdone"] == fm.HEAVY_GDONE
    assert amd.msm_front_plan("g1", 1 << 24)["plan"]["chunk"] == 128
    L, cfg, info = amd.lib(), amd.msm_config(), (ctypes.c_int64 * 29)()
    probe = lambda g, s, n, c, i, t: L.mbls_msm_front_probe(g, s, None, n, c, i, t)
    assert probe(1, None, 8, None, info, None) == amd.INVALID_POINTER
    assert probe(1, None, 8, ctypes.byref(cfg), None, None) == amd.INVALID_POINTER
    assert probe(3, None, 8, ctypes.byref(cfg), info, None) == amd.INVALID_ARGUMENT
    assert probe(1, None, 0, ctypes.byref(cfg), info, None) == amd.INVALID_ARGUMENT
    tables = (ctypes.c_void_p * len(amd.FRONT_TABLES))()
    assert probe(1, None, 8, ctypes.byref(cfg), info, tables) == amd.INVALID_POINTER  # tables without scalars
    cfg.batch_size = 2
    assert probe(1, None, 8, ctypes.byref(cfg), info, None) == amd.INVALID_ARGUMENT


def test_no_plan_has_512_segments_below_2_18(amd):
    """the side of k_part_sort's register-kept branch that DESIGN.md's census table lists as
    unreached at n <= 2^18, over every plan a caller can get there: a team walks because it owns
    more than PS_RS segments only with more than PS_RS teams' worth of segments in a window group"""
    n, seen = 1 << 18, 0
    for group in ("g1", "g2"):
        for F in range(1, 65):
            for c in [0] + list(range(2, 21)):
                for bits in (0, 128, 192):
                    try:
                        plan = amd.msm_front_plan(group, n, c=c, precompute_factor=F, bitsize=bits)["plan"]
                    except amd.IcicleError:
                        continue
                    if plan["partition_sort"]:
                        seen += 1
                        segments = ((plan["W"] - 1) // plan["Wg"] + 1) * fm.sort_sizes(plan)["tiles"]
                        assert segments <= fm.PS_RS * (fm.PS_THREADS // fm.PS_TEAM), plan
    assert seen > 1000


def test_glv_and_psi_digit_signs_follow_the_split(amd):
    """stream j's digits carry the sign of the split's half / quarter"""
    for name, dec in (("plan_glv_c16", lambda s: [(m, n) for m, n in zip(*[iter(fm.pr.glv_decompose(s))] * 2)]),
                      ("plan_psi_c13", fm.pr.psi_decompose)):
        case = fc.BY_NAME[name]
        plan, _ = designed_plan(amd, case)
        scalars = case.scalars()
        D = fm.model_digits(plan, scalars)
        for i in (0, 5, case.n - 1):
            for j, (mag, neg) in enumerate(dec(scalars[i] % fm.pr.R)):
                row = D[fm.stream_index(plan, j, i)]
                assert sum(int(d) << (plan["c"] * l) for l, d in enumerate(row)) == (-mag if neg else mag)


# ----------------------------------------------------------------------------- mutations
@pytest.fixture(scope="module")
def correct(amd):
    case = fc.BY_NAME["chunks_fused"]
    scalars = case.scalars() + [fc.dig(-9, 5)]  # one negative digit, with its carry
    info = amd.msm_front_plan(case.group, len(scalars), **case.cfg)
    plan, words = info["plan"], info["words"]
    D = fm.model_digits(plan, scalars)
    t = fm.model_tables(plan, D, words)
    fm.check(t, plan, scalars)
    return plan, words, scalars, t


def _entries(plan, t):
    TB = plan["TB"]
    off = t["offsets"][:TB + 1].astype(np.int64)
    return t["sorted"][:off[TB]].astype(np.int64), off


def _busy(off, k=0):
    """the k-th bucket holding at least two entries whose successor holds some too"""
    cnt = np.diff(off)
    return int(np.flatnonzero((cnt[:-1] >= 2) & (cnt[1:] >= 1))[k])


def move_entry(plan, words, t):
    e, off = _entries(plan, t)
    off[_busy(off) + 1] -= 1  # the bucket's last entry now opens the next bucket
    return fm.complete(plan, e, off, words)


def drop_entry(plan, words, t):
    e, off = _entries(plan, t)
    b = _busy(off)
    off[b + 1:] -= 1
    return fm.complete(plan, np.delete(e, off[b]), off, words)


def duplicate_entry(plan, words, t):
    e, off = _entries(plan, t)
    b = _busy(off)
    off[b + 1:] += 1
    return fm.complete(plan, np.insert(e, off[b], e[off[b]]), off, words)


def flip_sign(plan, words, t):
    t["sorted"][3] ^= 1
    return t


def offsets_decrease(plan, words, t):
    e, off = _entries(plan, t)
    b = _busy(off, 1)
    t["offsets"][b + 1] = off[b] - 1
    return t


def offsets_shift(plan, words, t):
    e, off = _entries(plan, t)
    t["offsets"][_busy(off) + 1] += 1
    return t


def offsets_total(plan, words, t):
    t["offsets"][plan["TB"]] -= 1
    return t


def chunk_off_by_one(plan, words, t):
    t["chunk_off"][_busy(_entries(plan, t)[1]) + 1] += 1
    return t


def nchunks_by_one(plan, words, t):
    t["nchunks"][_busy(_entries(plan, t)[1])] += 1
    return t


def nchunks_maximum(plan, words, t):
    t["nchunks"][plan["TB"]] -= 1
    return t


def owner_swap(plan, words, t):
    k = int(t["chunk_off"][_busy(_entries(plan, t)[1]) + 1])  # the first chunk of the next bucket
    t["owner"][[k - 1, k]] = t["owner"][[k, k - 1]]
    return t


def first_shift(plan, words, t):
    k = int(np.flatnonzero(t["first"] == fm.FILL)[0])
    t["first"][1:k] = t["first"][:k - 1].copy()
    return t


def perm_twice(plan, words, t):
    k = int(t["binbase"][fm.order_words(plan["TB"]) - 1]) - 3  # inside a slice of several buckets
    assert t["perm"][k] != t["perm"][k + 1]
    t["perm"][k] = t["perm"][k + 1]
    return t


def binbase_by_one(plan, words, t):
    t["binbase"][5] += 1
    return t


def heavy_omitted(plan, words, t):
    TB = plan["TB"]
    hc = int(t["nchunks"][TB + 1])
    last = int(np.flatnonzero(t["H_first"][:hc] == t["H_first"][:hc].max())[0])
    assert last == hc - 1  # the model lists them in bucket order: drop the last entry and its slices
    t["nchunks"][TB + 1] -= 1
    t["nchunks"][TB + 2] -= t["H_nslices"][last]
    for name in ("H_bucket", "H_first", "H_nslices", "H_done"):
        t[name][last] = fm.FILL
    t["H_owner"][t["H_owner"] == last] = fm.FILL
    return t


def heavy_replaced(plan, words, t):
    t["H_bucket"][1] = t["H_bucket"][0]
    return t


def heavy_overlap(plan, words, t):
    t["H_first"][1] = t["H_first"][0]
    return t


def heavy_owner(plan, words, t):
    t["H_owner"][1] = 0
    return t


def heavy_done(plan, words, t):
    t["H_done"][0] = 1
    return t


def group_counter(plan, words, t):
    t["H_gdone"][fm.HEAVY_GDONE - 1] = 3
    return t


def stale_tail(name):
    def mutate(plan, words, t):
        t[name][-1] = 0
        return t
    mutate.__name__ = f"stale_{name}"
    return mutate


MUTATIONS = [(move_entry, "sorted"), (drop_entry, "sorted"), (duplicate_entry, "sorted"), (flip_sign, "sorted"),
             (offsets_decrease, "offsets"), (offsets_shift, "sorted"), (offsets_total, "offsets"),
             (chunk_off_by_one, "chunk_off"), (nchunks_by_one, "nchunks"), (nchunks_maximum, "nchunks"),
             (owner_swap, "owner"), (first_shift, "first"), (perm_twice, "perm"), (binbase_by_one, "binbase"),
             (heavy_omitted, "H.cnt"), (heavy_replaced, "H.bucket"), (heavy_overlap, "H.first"), (heavy_owner, "H.owner"),
             (heavy_done, "H.done"), (group_counter, "H.gdone"), (stale_tail("sorted"), "sorted"),
             (stale_tail("owner"), "owner"), (stale_tail("first"), "first"), (stale_tail("perm"), "perm"),
             (stale_tail("H_owner"), "H.owner")]


@pytest.mark.parametrize("mutate,table", MUTATIONS, ids=[m.__name__ for m, _ in MUTATIONS])
def test_check_rejects_the_mutant(correct, mutate, table):
    plan, words, scalars, t = correct
    mutant = mutate(plan, words, {k: v.copy() for k, v in t.items()})
    assert any((mutant[k] != t[k]).any() for k in t), "the mutation changed nothing"
    with pytest.raises(fm.FrontMismatch) as e:
        fm.check(mutant, plan, scalars)
    assert e.value.table == table, str(e.value)
