#!/usr/bin/env python3
"""Extended-coset transform timing (device events on one stream, device-resident operands) at
extended_size = 2^22 with size = 2^20 (E = 2) and 2^19 (E = 3), g = zeta:

  forward  new       mbls_fr_coeff_to_extended
           composed  what a caller does without it: clear the tail of an N-element buffer
                     (hipMemsetAsync), copy the coefficients in (device copy), bls12_381_coset_ntt_cuda
           plain     bls12_381_ntt_cuda at 2^22: the floor
  inverse  new       mbls_fr_extended_to_coeff with vanishing_inv of period 2^E, out_size = 3 * size
           composed  bls12_381_vector_mul by the vanishing table expanded to N elements, inverse
                     bls12_381_coset_ntt_cuda; the truncation is a view and costs nothing
           plain     inverse bls12_381_ntt_cuda at 2^22

All from the same tree and process.  new and composed are compared once before the timing (exact
equality).  One warm-up, then --reps rounds of --iters back-to-back calls per leg, the legs
alternating; prints the median, min and max time per call.  There is no pass / fail bound.
--out FILE also writes the lines there.  MBLS_LIB selects another in-tree build."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=22, help="log2 of the extended size")
    ap.add_argument("--ext", type=int, nargs="*", default=[2, 3], help="extension bits E")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "midnight-bls12-381-cuda_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import bls12_381_amd as amd
    import domain_model as D

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {amd.lib().mbls_version().decode()} lib {os.path.relpath(amd.LIB_PATH, ROOT)} "
        f"device {torch.cuda.get_device_name(0)}")
    amd.ntt_init_domain()
    N = 1 << a.logn
    zeta = D.mont_words(D.ZETA)
    new = lambda rows=N: amd.torch_u64((rows, 4))
    x, vsrc = new(), new()
    amd.gen_scalars(x, 0xD0, montgomery=True)
    amd.gen_scalars(vsrc, 0xD1, montgomery=True)
    pad, o_new, o_comp, tmp = new(), new(), new(), new()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    def run(title, legs):
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
            say(f"{title} {k}: median {med[k]:.4f} ms min {v[0]:.4f} max {v[-1]:.4f} per call")
        say(f"{title} composed / new {med['composed'] / med['new']:.2f}, new / plain {med['new'] / med['plain']:.2f}")

    for E in a.ext:
        size, m = N >> E, min(N, 3 * (N >> E))
        coeffs = x[:size]
        plan = amd.domain_plan(size, N)
        say(f"# 2^{a.logn}, size 2^{a.logn - E} (E = {E}), out_size {m}: " + ", ".join(f"{k} {v}" for k, v in plan.items()))

        def f_new():
            amd.coeff_to_extended(coeffs, N, zeta, out=o_new, is_async=True)

        def f_comp():
            pad[size:].zero_()
            pad[:size].copy_(coeffs)
            amd.ntt(pad, out=o_comp, coset_gen=zeta, entry="coset", is_async=True)

        def f_plain():
            amd.ntt(x, out=tmp, is_async=True)

        f_new()
        f_comp()
        torch.cuda.synchronize()
        assert torch.equal(o_new, o_comp), "forward: new != composed"
        say(f"# forward E = {E}: new and composed outputs are equal")
        run(f"domain 2^{a.logn} E={E} forward", {"new": f_new, "composed": f_comp, "plain": f_plain})

        vinv = vsrc[:1 << E].clone()
        vfull = vinv.repeat(N >> E, 1).contiguous()
        co = new(m)

        def i_new():
            amd.extended_to_coeff(x, m, zeta, vinv, out=co, is_async=True)

        def i_comp():
            amd.vec_op("mul", x, vfull, out=tmp, is_async=True)
            amd.ntt(tmp, inverse=True, out=o_comp, coset_gen=zeta, entry="coset", is_async=True)

        def i_plain():
            amd.ntt(x, inverse=True, out=pad, is_async=True)

        i_new()
        i_comp()
        torch.cuda.synchronize()
        assert torch.equal(co, o_comp[:m]), "inverse: new != composed"
        say(f"# inverse E = {E}: new and composed outputs are equal")
        run(f"domain 2^{a.logn} E={E} inverse", {"new": i_new, "composed": i_comp, "plain": i_plain})
        del vfull, co

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
