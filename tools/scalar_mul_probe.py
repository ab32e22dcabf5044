#!/usr/bin/env python3
"""Batch scalar multiplication timing (device events, device-resident operands), G1 and G2 at
n = 2^16 and 2^20:

  candidate   scalar_mul + projective_to_affine (ends in Montgomery affine points)
  comparator  mbls_gen_g*_bases, the fixed-base 255-bit bit-serial multiplication with one
              inversion per point (also ends in Montgomery affine points)

One warm-up, then --reps timed rounds with the legs interleaved; prints median and min per leg.
--pkg DIR imports the binding from another checkout's package directory (to time the comparator
on the parent commit); --comparator-only skips the candidate (a checkout without scalar_mul)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--logn", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--groups", nargs="*", default=["g1", "g2"])
    ap.add_argument("--pkg", default=os.path.join(ROOT, "midnight-bls12-381-cuda_amd"))
    ap.add_argument("--comparator-only", action="store_true")
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

    for group in a.groups:
        nl = 12 if group == "g1" else 24
        for logn in a.logn:
            n = 1 << logn
            s = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
            b = torch.zeros((n, nl), dtype=torch.int64, device="cuda")
            amd.gen_scalars(s, 0x5EED0021, montgomery=False)
            amd.gen_bases(group, b, 0x5EED0022)
            jac = torch.zeros((n, nl * 3 // 2), dtype=torch.int64, device="cuda")
            aff = torch.zeros((n, nl), dtype=torch.int64, device="cuda")
            gen = torch.zeros((n, nl), dtype=torch.int64, device="cuda")
            legs = {"gen_bases": lambda: amd.gen_bases(group, gen, 0x5EED0023)}
            if not a.comparator_only:
                legs["scalar_mul"] = lambda: amd.scalar_mul(group, b, s, out=jac, is_async=True)
                legs["to_affine"] = lambda: amd.convert_points(group, "to_affine", jac, out=aff, is_async=True)
            ts = {k: [] for k in legs}
            for rep in range(a.reps + 1):
                for k, fn in legs.items():
                    t = timed(fn)
                    if rep:
                        ts[k].append(t)
            line = f"{group} 2^{logn}:"
            med = {}
            for k, v in ts.items():
                v.sort()
                med[k] = v[len(v) // 2]
                line += f" {k} median {med[k]:.3f} ms min {v[0]:.3f}"
            if "scalar_mul" in med:
                cand = med["scalar_mul"] + med["to_affine"]
                line += f" | candidate {cand:.3f} ms, comparator / candidate {med['gen_bases'] / cand:.2f}x"
            print(line, flush=True)


if __name__ == "__main__":
    main()
