#!/usr/bin/env python3
"""Expression evaluator timing (device events on one stream, device-resident operands) at 2^22 rows:

  fused     mbls_fr_eval_program, the two-output permutation program for m columns (default 3):
            num = prod_k (v_k + beta delta^k X + gamma), den = prod_k (v_k + beta sigma_k + gamma)
  composed  the same two columns from bls12_381_scalar_mul_vec / scalar_add_vec / vector_add /
            vector_mul, one launch and one pass over memory per operator

Both from the same tree and process.  The results are compared once before the timing (exact
equality).  One warm-up, then --reps rounds of --iters back-to-back calls per leg, the legs
alternating; prints the median, min and max time per call, the bytes each form moves by its
operators' own traffic (not a measured counter) and the rate that makes.  There is no pass / fail
bound.  --out FILE also writes the lines there.  MBLS_LIB selects another in-tree build."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=22)
    ap.add_argument("--m", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "midnight-bls12-381-cuda_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import bls12_381_amd as amd
    import expr_model as E

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {amd.lib().mbls_version().decode()} lib {os.path.relpath(amd.LIB_PATH, ROOT)} "
        f"device {torch.cuda.get_device_name(0)}")
    n, m = 1 << a.logn, a.m
    new = lambda rows=n: amd.torch_u64((rows, 4))
    cols = [new() for _ in range(2 * m + 1)]  # v_0 .., sigma_0 .., X
    for k, c in enumerate(cols):
        amd.gen_scalars(c, 0xE0 + k, montgomery=True)
    consts = new(m + 2)  # beta delta^k .., beta, gamma
    amd.gen_scalars(consts, 0xEC, montgomery=True)
    prog = E.permutation(m)
    info = amd.expr_check(prog, 2 * m + 1, m + 2, 2)
    say(f"# program: {len(prog)} ops, " + ", ".join(f"{k} {v}" for k, v in info.items()))
    fused_out = new(2 * n)
    t1, t2, fac = new(), new(), new()
    prods = [[new(), new()], [new(), new()]]  # per side, the running product alternates between two buffers

    def fused():
        amd.eval_program(cols, prog, constants=consts, n_outputs=2, out=fused_out, is_async=True)

    passes = []  # bytes per row of every composed operator

    def op(name, x, y, out, cost):
        amd.vec_op(name, x, y, out=out, is_async=True)
        passes.append(cost)

    def composed():
        """no operator writes over one of its inputs; the scalars are device elements, so nothing is
        staged; returns the two result buffers"""
        del passes[:]
        res = []
        for side in range(2):
            for k in range(m):
                dst = prods[side][0] if k == 0 else fac
                # beta delta^k X or beta sigma_k, + v_k, + gamma, then into the running product
                op("scalar_mul", consts[k:k + 1] if side == 0 else consts[m:m + 1], cols[2 * m] if side == 0 else cols[m + k],
                   t1, 64)
                op("add", t1, cols[k], t2, 96)
                op("scalar_add", consts[m + 1:m + 2], t2, dst, 64)
                if k:
                    op("mul", prods[side][(k - 1) & 1], fac, prods[side][k & 1], 96)
            res.append(prods[side][(m - 1) & 1])
        return res

    fused()
    comp_num, comp_den = composed()
    torch.cuda.synchronize()
    assert torch.equal(fused_out[:n], comp_num) and torch.equal(fused_out[n:], comp_den), "fused != composed"
    say("# fused and composed outputs are equal")
    bytes_row = {"fused": (2 * m + 1 + 2) * 32, "composed": sum(passes)}
    launches = {"fused": 1, "composed": len(passes)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    legs = {"fused": fused, "composed": composed}
    ts = {k: [] for k in legs}
    for rep in range(a.reps + 1):  # round 0 is the warm-up
        for k, fn in legs.items():
            t = timed(fn)
            if rep:
                ts[k].append(t)
    med = {}
    for k, v in ts.items():
        v.sort()
        med[k] = v[len(v) // 2]
        gb = bytes_row[k] * n / 1e9
        say(f"expr 2^{a.logn} m={m} {k}: median {med[k]:.4f} ms min {v[0]:.4f} max {v[-1]:.4f} per call, "
            f"{launches[k]} launches, {bytes_row[k]} B/row = {gb:.3f} GB moved, {gb / med[k]:.2f} TB/s")
    say(f"expr 2^{a.logn} m={m} composed / fused time {med['composed'] / med['fused']:.2f}, "
        f"bytes {bytes_row['composed'] / bytes_row['fused']:.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
