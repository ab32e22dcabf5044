"""The MSM front's tables on the device against the contract model (tests/front_model.py), from
both sides of each of the front's branches (tests/front_cases.py; DESIGN.md "The front's contract"
has the census table).  mbls_msm_front_probe runs what an MSM runs up to the front -- the same plan,
chunk length, staging and scratch region, filled with 0xA5 first -- and returns every table at its
block's full capacity.  Each case first asserts the plan fields it was designed for and its cell of
the branch census, then check(): exact comparisons only, nothing skipped or filtered.

tests/test_front_model.py runs the same cases through the model alone, and the mutation checks of
the checker, without a GPU."""
import numpy as np
import pytest

import helpers as H
import front_cases as fc
import front_model as fm
from helpers import pyref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gpu_helpers
    gpu_helpers.amd.lib()
    return gpu_helpers.amd


def run_front(amd, case, scalars=None, stream=None):
    """the case's plan and census cell, then its tables from the device"""
    import torch
    scalars = case.scalars() if scalars is None else scalars
    info = amd.msm_front_plan(case.group, len(scalars), **case.cfg)
    plan = info["plan"]
    assert {k: plan[k] for k in case.plan} == case.plan, f"{case.name} no longer runs the plan it was designed for"
    std = [s % pr.R for s in scalars] if case.mont else scalars
    limbs = H.ints_to_limbs([pr.fr_to_mont(s) for s in std] if case.mont else std, 4)
    bases = None
    if case.bases != "none":
        rows = len(scalars) * (case.cfg.get("precompute_factor", 1) if case.bases == "table" else 1)
        bases = torch.zeros((rows, 12 if case.group == "g1" else 24), dtype=torch.int64, device="cuda")
        amd.gen_bases(case.group, bases, 0xF207)
    out = amd.msm_front_tables(case.group, amd.torch_u64(limbs), bases, scalars_mont=case.mont, stream=stream, **case.cfg)
    assert out["plan"] == plan and {k: len(v) for k, v in out["tables"].items()} == info["words"]
    return out, std


@pytest.mark.parametrize("name", [k.name for k in fc.CASES])
def test_front_tables_meet_the_contract(amd, name):
    case = fc.BY_NAME[name]
    scalars = case.scalars()
    plan = amd.msm_front_plan(case.group, len(scalars), **case.cfg)["plan"]
    D = fm.model_digits(plan, scalars)
    z = fm.census(plan, D)
    assert case.cell(z), f"{name} left its census cell: {z}"
    out, std = run_front(amd, case, scalars)
    fm.check(out["tables"], out["plan"], std, digits=D)


def test_host_scalars_take_the_same_front(amd):
    """pageable host scalars (the staged copy) give the tables device scalars give, bucket by bucket;
    and the device's tables do not pass for other scalars: one scalar off by one, or two points
    exchanged, fails at `sorted`"""
    case = fc.BY_NAME["digit_edges"]
    scalars = case.scalars()
    out = amd.msm_front_tables(case.group, H.ints_to_limbs(scalars, 4), None, **case.cfg)
    fm.check(out["tables"], out["plan"], scalars)
    for other in (scalars[:5] + [scalars[5] + 1] + scalars[6:], scalars[:2] + [scalars[3], scalars[2]] + scalars[4:]):
        with pytest.raises(fm.FrontMismatch) as e:
            fm.check(out["tables"], out["plan"], other)
        assert e.value.table == "sorted"


def test_a_light_call_after_a_heavy_one_starts_clean(amd):
    """one stream, one plan, one size: a call with a heavy part (helpers planned, hh and hpart
    written), then a light call over the same arena region.  The 0xA5 fill and the second check show
    that part_tot, the order histograms, the three words at nchunks[TB..], H.gdone and the helper
    plan are re-established per call and nothing is carried over."""
    import torch
    heavy, light = fc.BY_NAME["part_above_PH_MIN"], fc.BY_NAME[f"tiles_{2 * fm.DT_TILE + 1}"]
    assert heavy.n == light.n and heavy.cfg == light.cfg
    st = torch.cuda.Stream()
    a, sa = run_front(amd, heavy, stream=st)
    fm.check(a["tables"], a["plan"], sa)
    assert int(a["tables"]["nchunks"][a["plan"]["TB"] + 1]) > 0  # the heavy call listed heavy buckets
    b, sb = run_front(amd, light, stream=st)
    fm.check(b["tables"], b["plan"], sb)
    c, sc = run_front(amd, heavy, stream=st)
    fm.check(c["tables"], c["plan"], sc)
    for k in ("offsets", "nchunks", "chunk_off", "owner", "first", "binbase"):  # order-free tables repeat exactly
        assert np.array_equal(a["tables"][k], c["tables"][k]), k
