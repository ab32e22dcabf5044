#!/usr/bin/env python3
"""Fr inner-product timing (device events, device-resident operands) at n = 2^20 and 2^22 rows:

  evaluation phase   multi_eval_32x3   mbls_fr_multi_eval, 32 columns at 3 points
                     inner_32x3        mbls_fr_inner_products over the 3 power vectors already in
                                       memory: multi_eval without its powers
                     scans_32x3        the best existing route: three batched evaluation-only
                                       mbls_fr_poly_divide_linear calls (batch 32, one point each;
                                       two of batch 16 per point at 2^22, a call taking 2^26 elements)
  plain product      inner_32x1        mbls_fr_inner_products, 32 columns by 1 vector
                     mul_sum_32x1      32 bls12_381_vector_mul into one array, one batched
                                       bls12_381_vector_sum
  powers fill        powers            mbls_fr_powers, one member
                     prefix_const      mbls_fr_prefix_product over a constant column
  crossover          multi_eval_1x1    one column at one point
                     scan_1x1          one evaluation-only mbls_fr_poly_divide_linear

All from the same tree and process.  The outputs of each pair are compared first.  One warm-up, then
--reps timed rounds with the legs interleaved; prints median, min and max per leg, the ratios of
each pair and the products and bytes per second the new calls reach.  There is no pass / fail bound.
MBLS_LIB selects another in-tree build of the library."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC, NP = 32, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--logn", type=int, nargs="*", default=[20, 22])
    ap.add_argument("--pkg", default=os.path.join(ROOT, "midnight-bls12-381-cuda_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
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

    for logn in a.logn:
        n = 1 << logn
        print(f"# 2^{logn} plan 32x3 " + " ".join(f"{k} {v}" for k, v in amd.inner_plan(n, NC, NP).items()), flush=True)
        allc, tmp = amd.torch_u64((NC * n, 4)), amd.torch_u64((NC * n, 4))
        amd.gen_scalars(allc, 0x1AE0, montgomery=True)
        cols = [allc[p * n:(p + 1) * n] for p in range(NC)]
        pts = amd.torch_u64((NP, 4))
        amd.gen_scalars(pts, 0x1AE1, montgomery=True)
        zrep = [pts[k:k + 1].repeat(NC, 1).contiguous() for k in range(NP)]
        pw = amd.powers(pts, n)
        vecs = [pw[k * n:(k + 1) * n] for k in range(NP)]
        const = pts[0:1].repeat(n, 1).contiguous()
        o_me, o_in, o_sc = amd.torch_u64((NC * NP, 4)), amd.torch_u64((NC * NP, 4)), [amd.torch_u64((NC, 4)) for _ in range(NP)]
        o_i1, o_ms = amd.torch_u64((NC, 4)), amd.torch_u64((NC, 4))
        o_pw, o_pp = amd.torch_u64((n, 4)), amd.torch_u64((n, 4))
        o_m1, o_s1 = amd.torch_u64((1, 4)), amd.torch_u64((1, 4))

        # a scan call takes at most 2^26 elements: the 32 columns go in `parts` calls per point
        parts = max(1, NC * n >> 26)
        per = NC // parts

        def scans():
            for k in range(NP):
                for q in range(parts):
                    amd.poly_divide_linear(allc[q * per * n:(q + 1) * per * n], zrep[k][:per], batch=per, quotient=False,
                                           eval=o_sc[k][q * per:(q + 1) * per], is_async=True)

        def mul_sum():
            for p in range(NC):
                amd.vec_op("mul", cols[p], vecs[0], out=tmp[p * n:(p + 1) * n], is_async=True)
            amd.vector_sum(tmp, batch=NC, out=o_ms, is_async=True)

        legs = {"multi_eval_32x3": lambda: amd.multi_eval(cols, pts, out=o_me, is_async=True),
                "inner_32x3": lambda: amd.inner_products(cols, vecs, out=o_in, is_async=True),
                "scans_32x3": scans,
                "inner_32x1": lambda: amd.inner_products(cols, vecs[:1], out=o_i1, is_async=True),
                "mul_sum_32x1": mul_sum,
                "powers": lambda: amd.powers(pts[0:1], n, out=o_pw, is_async=True),
                "prefix_const": lambda: amd.prefix_product(const, out=o_pp, is_async=True),
                "multi_eval_1x1": lambda: amd.multi_eval(cols[:1], pts[0:1], out=o_m1, is_async=True),
                "scan_1x1": lambda: amd.poly_divide_linear(cols[0], pts[0:1], quotient=False, eval=o_s1, is_async=True)}
        for fn in legs.values():  # the warm-up, and the outputs compared once
            fn()
        torch.cuda.synchronize()
        want = torch.stack(o_sc, dim=1).reshape(NC * NP, 4)
        assert torch.equal(o_me, want) and torch.equal(o_in, want), "multi_eval equals the evaluation-only scans"
        assert torch.equal(o_i1, o_ms) and torch.equal(o_i1, want[0::NP]), "inner product equals vector_mul + vector_sum"
        assert torch.equal(o_pw, o_pp) and torch.equal(o_pw, vecs[0]), "powers equal the running product of a constant"
        assert torch.equal(o_m1, o_s1) and torch.equal(o_m1, want[0:1]), "one column at one point"

        ts = {k: [] for k in legs}
        for rep in range(a.reps):
            for k, fn in legs.items():
                ts[k].append(timed(fn))
        med = {}
        for k, v in ts.items():
            v.sort()
            med[k] = v[len(v) // 2]
            print(f"inner 2^{logn}: {k} median {med[k]:.3f} ms min {v[0]:.3f} max {v[-1]:.3f}", flush=True)
        pairs = NC * NP * n
        print(f"inner 2^{logn}: scans_32x3 / multi_eval_32x3 {med['scans_32x3'] / med['multi_eval_32x3']:.2f}, "
              f"scans_32x3 / inner_32x3 {med['scans_32x3'] / med['inner_32x3']:.2f}, "
              f"mul_sum_32x1 / inner_32x1 {med['mul_sum_32x1'] / med['inner_32x1']:.2f}, "
              f"prefix_const / powers {med['prefix_const'] / med['powers']:.2f}, "
              f"scan_1x1 / multi_eval_1x1 {med['scan_1x1'] / med['multi_eval_1x1']:.2f}", flush=True)
        # multi_eval: 96 n products of the sums + 3 n of the powers; columns read ceil(3 / VB) times,
        # vectors once per column block if they miss the caches, powers written once
        plan = amd.inner_plan(n, NC, NP)
        nvb, ncb = -(-NP // plan["VB"]), -(-NC // plan["CB"])
        worst = 32 * n * (NC * nvb + NP * ncb)
        print(f"inner 2^{logn}: inner_32x3 {pairs / med['inner_32x3'] / 1e6:.1f} G products/s, "
              f"{32 * n * (NC * nvb + NP) / med['inner_32x3'] / 1e6:.1f} GB/s if the vectors are read once, "
              f"{worst / med['inner_32x3'] / 1e6:.1f} GB/s if once per column block; "
              f"inner_32x1 {NC * n / med['inner_32x1'] / 1e6:.1f} G products/s; "
              f"powers {n / med['powers'] / 1e6:.1f} G products/s, {32 * n / med['powers'] / 1e6:.1f} GB/s written", flush=True)
        del allc, tmp, pw, const


if __name__ == "__main__":
    main()
