#!/usr/bin/env python3
"""Fr scan timing (device events, device-resident operands) at n = 2^20 and 2^24:

  candidates   product      mbls_fr_prefix_product without den, device total
               product_den  mbls_fr_prefix_product with den (the ratio kernel, then the same scan)
               divide       mbls_fr_poly_divide_linear, quotient and evaluation
               evaluate     mbls_fr_poly_divide_linear, evaluation only (two launches, no vector written)
  comparators  mul          bls12_381_vector_mul at the same n: the one-product-per-element floor
               inv_mul      bls12_381_batch_inv_cuda then bls12_381_vector_mul: the work the den leg
                            fuses (num / den without the scan)

All from the same tree and process.  One warm-up, then --reps timed rounds with the legs
interleaved; prints median, min and max per leg and the ratios to mul.  The results are checked once
before the timing: out[i + 1] = out[i] * x[i] with vector_mul, and the evaluation-only leg against
the full one.  There is no pass / fail bound.  MBLS_LIB selects another in-tree build of the
library."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--logn", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--pkg", default=os.path.join(ROOT, "midnight-bls12-381-cuda_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import torch
    import bls12_381_amd as amd
    print(f"# {amd.lib().mbls_version().decode()} lib {os.path.relpath(amd.LIB_PATH, ROOT)} "
          f"device {torch.cuda.get_device_name(0)}", flush=True)
    print("# geometry " + " ".join(f"{k} {v}" for k, v in amd.scan_geometry(1).items() if k in ("K", "tile")), flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for logn in a.logn:
        n = 1 << logn
        x, d, z = amd.torch_u64((n, 4)), amd.torch_u64((n, 4)), amd.torch_u64((1, 4))
        amd.gen_scalars(x, 0x5CA0, montgomery=True)
        amd.gen_scalars(d, 0x5CA1, montgomery=True)
        amd.gen_scalars(z, 0x5CA2, montgomery=True)
        out, tmp = amd.torch_u64((n, 4)), amd.torch_u64((n, 4))
        tot, ev, ev2 = amd.torch_u64((1, 4)), amd.torch_u64((1, 4)), amd.torch_u64((1, 4))

        def inv_mul():
            amd.batch_inv(d, tmp)  # synchronous by its own contract: the events still bracket the device work
            amd.vec_op("mul", x, tmp, out=tmp, is_async=True)

        legs = {"product": lambda: amd.prefix_product(x, out=out, total=tot, is_async=True),
                "product_den": lambda: amd.prefix_product(x, d, out=out, total=tot, is_async=True),
                "divide": lambda: amd.poly_divide_linear(x, z, out=out, eval=ev, is_async=True),
                "evaluate": lambda: amd.poly_divide_linear(x, z, quotient=False, eval=ev2, is_async=True),
                "mul": lambda: amd.vec_op("mul", x, d, out=tmp, is_async=True),
                "inv_mul": inv_mul}
        # correctness once: the recurrence with vector_mul, the den leg against inv_mul's ratios
        legs["product"]()
        amd.vec_op("mul", out, x, out=tmp)
        assert torch.equal(tmp[:-1], out[1:]) and torch.equal(tmp[-1:], tot), "out[i+1] = out[i] * x[i]"
        inv_mul()
        ratios = tmp.clone()
        legs["product_den"]()
        amd.vec_op("mul", out, ratios, out=tmp)
        assert torch.equal(tmp[:-1], out[1:]) and torch.equal(tmp[-1:], tot), "out[i+1] = out[i] * x[i] / d[i]"
        legs["divide"]()
        legs["evaluate"]()
        torch.cuda.synchronize()
        assert torch.equal(ev, ev2), "evaluation only equals the full call's evaluation"

        ts = {k: [] for k in legs}
        for rep in range(a.reps + 1):
            for k, fn in legs.items():
                t = timed(fn)
                if rep:
                    ts[k].append(t)
        med = {}
        line = f"scan 2^{logn}:"
        for k, v in ts.items():
            v.sort()
            med[k] = v[len(v) // 2]
            line += f" {k} median {med[k]:.3f} ms min {v[0]:.3f} max {v[-1]:.3f}"
        m = ts["mul"]
        line += " |" + "".join(f" {k} / mul {med[k] / med['mul']:.2f}," for k in legs if k != "mul")
        line += f" product_den / inv_mul {med['product_den'] / med['inv_mul']:.2f}, mul spread {(m[-1] - m[0]) / med['mul']:.3f}"
        print(line, flush=True)
        del x, d, out, tmp, ratios


if __name__ == "__main__":
    main()
