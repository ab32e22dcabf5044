#!/usr/bin/env python3
"""Point validation timing (device events, device-resident operands) at n = 2^16 and 2^20 valid
points, both groups:

  candidate   check_points (mbls_g*_check_points), device points, device status, no count (a count
              is a host output and would make the call synchronous)
  comparator  scalar_mul (mbls_g*_scalar_mul) on the same points with a seeded stream of random
              scalars, device in, device out: the same kind of work per lane (one doubling chain
              per point), from the same tree

Valid points are the expensive input: a point that fails an earlier test leaves before the chain.
One warm-up, then --reps timed rounds with the legs interleaved in one process; prints median, min
and max per leg and the candidate / comparator ratio.  There is no pass / fail bound."""
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
            p = torch.zeros((n, nl), dtype=torch.int64, device="cuda")
            s = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
            amd.gen_bases(group, p, 0x5EED0041)
            amd.gen_scalars(s, 0x5EED0042, montgomery=False)
            status = torch.zeros((n,), dtype=torch.uint8, device="cuda")
            jac = torch.zeros((n, nl * 3 // 2), dtype=torch.int64, device="cuda")
            _, bad = amd.check_points(group, p, out=status)
            assert bad == 0 and not bool(status.any()), "generated bases must be valid"

            legs = {"check": lambda: amd.check_points(group, p, out=status, count=False, is_async=True),
                    "scalar_mul": lambda: amd.scalar_mul(group, p, s, out=jac, is_async=True)}
            ts = {k: [] for k in legs}
            for rep in range(a.reps + 1):
                for k, fn in legs.items():
                    t = timed(fn)
                    if rep:
                        ts[k].append(t)
            med = {}
            line = f"{group} check_points 2^{logn}:"
            for k, v in ts.items():
                v.sort()
                med[k] = v[len(v) // 2]
                line += f" {k} median {med[k]:.3f} ms min {v[0]:.3f} max {v[-1]:.3f}"
            c = ts["scalar_mul"]
            line += (f" | check / scalar_mul {med['check'] / med['scalar_mul']:.3f}, scalar_mul spread "
                     f"{(c[-1] - c[0]) / med['scalar_mul']:.3f}")
            print(line, flush=True)
            del p, s, status, jac


if __name__ == "__main__":
    main()
