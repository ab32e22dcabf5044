"""bench.py's multi-rank path, rehearsed on one GPU.

The driver's SCALE run launches `bench.py --gpus N` for N = 2, 4, 8 on a whole node; no multi-GPU
node is ours to use.  These tests run the same code path as child processes on the one-GPU box:
MBLS_BENCH_SAME_DEVICE=1 puts both ranks on device 0 and MBLS_BENCH_BACKEND=gloo replaces RCCL
(which refuses two ranks on one device).  Pinned: the rank launcher (bench.py launch_ranks), the
world-size bookkeeping of the JSON line, and sharded_msm.gather_partials' exchange + EC sum --
config #4's sharded MSM digest at N = 2 equals the N = 1 digest (the 1-GPU result is pinned to
the oracle by tests/test_gpu_parity.py)."""
import json
import os
import subprocess
import sys

import pytest

import helpers as H

pytestmark = pytest.mark.gpu
BENCH = os.path.join(H.ROOT, "bench.py")
# --full: config #4 (the sharded 2^21 MSM whose digest is compared) is one of its legs
ARGS = ["--full", "--msm-total-log", "21", "--steps", "2", "--warmup", "1", "--no-cpu", "--no-mix", "--msm-batch", "0",
        "--no-stage-profile"]


def _run(gpus, extra_env=None, timeout=240, args=ARGS):
    env = dict(os.environ)
    env.update(extra_env or {})
    p = subprocess.run([sys.executable, BENCH, "--gpus", str(gpus)] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    line = None
    for ln in p.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = json.loads(ln)
    return p.returncode, line, p.stderr[-2000:]


@pytest.fixture(scope="module")
def n1():
    rc, line, err = _run(1)
    assert rc == 0 and line, err
    return line


def test_bench_two_ranks_same_device_matches_one(n1):
    rc, line, err = _run(2, {"MBLS_BENCH_SAME_DEVICE": "1", "MBLS_BENCH_BACKEND": "gloo"})
    assert rc == 0 and line, err
    assert line["n_gpus"] == 2
    assert len(line["rank_devices"]) == 2 and sorted(d["rank"] for d in line["rank_devices"]) == [0, 1]
    assert line["config"]["parallelism"] == "msm-shard2"
    a, b = line["config4_msm_sharded"], n1["config4_msm_sharded"]
    assert a["result_digest"] == b["result_digest"], (a, b)
    # weak scaling: every rank ran the headline MSM on its own 2^20 points
    assert line["config"]["msm_points_per_gpu"] == n1["config"]["msm_points_per_gpu"]


def test_bench_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """without --full: the timed steps only (none of --full's fields in the line), and --dump-outputs
    writes the last step's G1 point, (x, y, 1) as 36 32-bit words in float64 -- equal to the same
    call on the same seeded inputs made here"""
    import numpy as np
    import torch
    import gpu_helpers
    amd = gpu_helpers.amd
    rc, line, err = _run(1, args=["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")])
    assert rc == 0 and line, err
    assert line["full"] is False and line["steps"] == 3 and line["msm_step_ms"]["n"] == 3
    assert line["unit"] == "MSM/s" and line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
    for k in ("ntt_per_sec", "msm_stage_ms", "roofline", "config4_msm_sharded", "cpu_baseline", "vecops",
              "msm_raw_entry_per_sec", "mix_g2msm_batched_ntt"):
        assert k not in line, k
    assert sorted(os.listdir(tmp_path / "dump")) == ["g1_msm_result.npy"]
    got = np.load(tmp_path / "dump" / "g1_msm_result.npy")
    assert got.dtype == np.float64 and got.shape == (1, 36)
    n = 1 << 20
    s = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    amd.gen_scalars(s, 0x5EED0003, montgomery=True)
    b = torch.zeros((n, 12), dtype=torch.int64, device="cuda")
    amd.gen_bases("g1", b, 0x5EED0013)
    out = torch.zeros((1, 18), dtype=torch.int64, device="cuda")
    amd.msm("g1", s, b, icicle=True, scalars_mont=True, out=out, n=n)
    torch.cuda.synchronize()
    want = np.ascontiguousarray(amd.to_numpy_u64(out)).view(np.uint32).astype(np.float64)
    assert np.array_equal(got, want)


def test_bench_refuses_more_ranks_than_gpus():
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has 2+ GPUs: the refusal path is not reachable")
    rc, line, err = _run(2, timeout=120)
    assert rc == 2 and line is None, (rc, err)
    assert "needs 2 visible GPUs" in err
