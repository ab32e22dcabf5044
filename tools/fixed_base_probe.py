#!/usr/bin/env python3
"""Fixed-base multiplication timing (device events, device-resident operands).

Per group (G1, G2) and n = 2^16, 2^20, every leg ending in canonical Montgomery affine points:

  fixed_base   mbls_g*_fixed_base_mul over the table of one base
  variable     mbls_g*_scalar_mul on n copies of the base + projective_to_affine (the only route
               without the table)
  table        mbls_g*_fixed_base_table (once per base)

and for the G1 SRS, per n:

  lagrange     mbls_g1_srs_from_secret(basis 1)
  monomial     mbls_g1_srs_from_secret(basis 0)
  ecntt        mbls_g1_ecntt(inverse) of the monomial SRS (monomial + ecntt is the other route to
               the Lagrange SRS)

One warm-up, then --reps timed rounds with the legs interleaved in one process; prints median and
min per leg, and the plan the library reports.  MBLS_LIB selects another in-tree build of the
library (a build with another digit width, to compare widths in one job)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--logn", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--groups", nargs="*", default=["g1", "g2"])
    ap.add_argument("--no-srs", action="store_true")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "midnight-bls12-381-cuda_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import numpy as np
    import torch
    import bls12_381_amd as amd
    print(f"# {amd.lib().mbls_version().decode()} lib {os.path.relpath(amd.LIB_PATH, ROOT)} "
          f"device {torch.cuda.get_device_name(0)}", flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def run(title, legs, reps, derive=None):
        ts = {k: [] for k in legs}
        for rep in range(reps + 1):
            for k, fn in legs.items():
                t = timed(fn)
                if rep:
                    ts[k].append(t)
        line, med = title + ":", {}
        for k, v in ts.items():
            v.sort()
            med[k] = v[len(v) // 2]
            line += f" {k} median {med[k]:.3f} ms min {v[0]:.3f}"
        if derive:
            line += " | " + derive(med)
        print(line, flush=True)

    tables = {}
    for group in a.groups:
        nl = 12 if group == "g1" else 24
        plan = amd.fixed_base_plan(group)
        print(f"# {group} plan {plan}", flush=True)
        base = torch.zeros((1, nl), dtype=torch.int64, device="cuda")
        amd.gen_bases(group, base, 0x5EED0031)
        tables[group] = amd.fixed_base_table(group, base)
        run(f"{group} table", {"table": lambda: amd.fixed_base_table(group, base, is_async=True)}, a.reps)
        for logn in a.logn:
            n = 1 << logn
            s = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
            amd.gen_scalars(s, 0x5EED0032, montgomery=False)
            rep_b = base.repeat(n, 1).contiguous()
            jac = torch.zeros((n, nl * 3 // 2), dtype=torch.int64, device="cuda")
            aff = torch.zeros((n, nl), dtype=torch.int64, device="cuda")
            out = torch.zeros((n, nl), dtype=torch.int64, device="cuda")
            tab = tables[group]

            def variable():
                amd.scalar_mul(group, rep_b, s, out=jac, is_async=True)
                amd.convert_points(group, "to_affine", jac, out=aff, is_async=True)

            run(f"{group} 2^{logn}",
                {"fixed_base": lambda: amd.fixed_base_mul(group, tab, s, out=out, is_async=True), "variable": variable},
                a.reps, lambda m: f"variable / fixed_base {m['variable'] / m['fixed_base']:.2f}x")
            torch.cuda.synchronize()
            assert torch.equal(out, aff), "the two routes disagree"
            del s, rep_b, jac, aff, out
    if a.no_srs or "g1" not in tables:
        return
    tau = np.array([0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111111122222222, 0x0333333344444444], dtype=np.uint64)
    for logn in a.logn:
        n = 1 << logn
        lag = torch.zeros((n, 12), dtype=torch.int64, device="cuda")
        mono = torch.zeros((n, 12), dtype=torch.int64, device="cuda")
        via = torch.zeros((n, 12), dtype=torch.int64, device="cuda")
        tab = tables["g1"]
        amd.srs_from_secret(tab, tau, n, out=mono)
        run(f"srs 2^{logn}",
            {"lagrange": lambda: amd.srs_from_secret(tab, tau, n, lagrange=True, out=lag, is_async=True),
             "monomial": lambda: amd.srs_from_secret(tab, tau, n, out=mono, is_async=True),
             "ecntt": lambda: amd.ecntt(mono, inverse=True, out=via, is_async=True)},
            a.reps, lambda m: f"(monomial + ecntt) / lagrange {(m['monomial'] + m['ecntt']) / m['lagrange']:.1f}x")
        torch.cuda.synchronize()
        assert torch.equal(lag, via), "the two routes disagree"


if __name__ == "__main__":
    main()
