#!/usr/bin/env python3
"""G1 EC-NTT timing (device events, device-resident operands) at n = 2^16 and 2^20, forward and
inverse:

  candidate   ecntt (mbls_g1_ecntt), device in, device out
  comparator  what the public entries without it can do for the same job: per stage one scalar_mul
              of n/2 pairs plus one projective_to_affine of n points, k stages -- the
              multiplication and normalisation work with no butterfly additions and no skipped
              trivial twiddles (the scalars are a seeded stream: the cost does not depend on them)

One warm-up, then --reps timed rounds with the legs interleaved in one process; prints median, min
and max per leg and the candidate / comparator ratios."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--logn", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--pkg", default=os.path.join(ROOT, "midnight-bls12-381-cuda_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import torch
    import bls12_381_amd as amd
    print(f"# {amd.lib().mbls_version().decode()} pkg {os.path.relpath(a.pkg, ROOT)} "
          f"device {torch.cuda.get_device_name(0)}", flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for logn in a.logn:
        n = 1 << logn
        p = torch.zeros((n, 12), dtype=torch.int64, device="cuda")
        s = torch.zeros((n // 2, 4), dtype=torch.int64, device="cuda")
        amd.gen_bases("g1", p, 0x5EED0031)
        amd.gen_scalars(s, 0x5EED0032, montgomery=False)
        half = p[:n // 2]
        out = torch.zeros_like(p)
        jac = torch.zeros((n, 18), dtype=torch.int64, device="cuda")
        aff = torch.zeros_like(p)
        amd.scalar_mul("g1", half, s, out=jac[n // 2:])  # the upper half stays: no identity is normalised

        def comparator():
            for _ in range(logn):
                amd.scalar_mul("g1", half, s, out=jac[:n // 2], is_async=True)
                amd.convert_points("g1", "to_affine", jac, out=aff, is_async=True)

        legs = {"forward": lambda: amd.ecntt(p, out=out, is_async=True),
                "comparator": comparator,
                "inverse": lambda: amd.ecntt(p, inverse=True, out=out, is_async=True)}
        ts = {k: [] for k in legs}
        for rep in range(a.reps + 1):
            for k, fn in legs.items():
                t = timed(fn)
                if rep:
                    ts[k].append(t)
        med = {}
        line = f"g1 ecntt 2^{logn}:"
        for k, v in ts.items():
            v.sort()
            med[k] = v[len(v) // 2]
            line += f" {k} median {med[k]:.3f} ms min {v[0]:.3f} max {v[-1]:.3f}"
        c = ts["comparator"]
        line += (f" | forward / comparator {med['forward'] / med['comparator']:.3f}, inverse / comparator "
                 f"{med['inverse'] / med['comparator']:.3f}, comparator spread {(c[-1] - c[0]) / med['comparator']:.3f}")
        print(line, flush=True)


if __name__ == "__main__":
    main()
