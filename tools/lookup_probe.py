#!/usr/bin/env python3
"""Fr sort and lookup-permute timing (device events, device-resident Montgomery operands) at
n = 2^16, 2^20 and 2^22, for two kinds of column:

  full    full-width random elements; the lookup's input draws n rows of the table at random
  range16 a 16-bit range table (0 .. 2^16 - 1, padded with zeros) and random 16-bit inputs: after
          from_mont only the lowest key word varies, so seven of the eight words are skipped

  candidates   sort     mbls_fr_sort, sorted elements only
               lookup   mbls_fr_lookup_permute without the count (asynchronous)
  comparator   mul      bls12_381_vector_mul at the same n: the scale of one pass over a column

All from the same tree and process.  One warm-up, then --reps timed rounds with the legs interleaved;
prints median, min and max per leg, the ratios to mul and the launches per call (counted from
mbls_fr_sort_plan, memsets included).  The results are checked once before the timing: the sorted
column is ascending under the model's order on a sample and is a permutation (perm is one), and the
lookup reports no missing value.  There is no pass / fail bound.  MBLS_LIB selects another in-tree
build of the library (the uniform-word A/B)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--logn", type=int, nargs="*", default=[16, 20, 22])
    ap.add_argument("--pkg", default=os.path.join(ROOT, "midnight-bls12-381-cuda_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import torch
    import bls12_381_amd as amd
    print(f"# {amd.lib().mbls_version().decode()} lib {os.path.relpath(amd.LIB_PATH, ROOT)} "
          f"device {torch.cuda.get_device_name(0)}", flush=True)
    r2 = np.frombuffer(pow(2, 512, R).to_bytes(32, "little"), dtype=np.uint64).reshape(1, 4).copy()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def to_mont(std):
        return amd.vec_op("scalar_mul", r2, std, out=amd.torch_u64((std.shape[0], 4)))  # x * R^2 / R

    def small(vals):
        t = amd.torch_u64((vals.shape[0], 4))
        t[:, 0] = vals
        return to_mont(t)

    for logn in a.logn:
        n = 1 << logn
        plan = amd.sort_plan(n)
        plan2 = amd.sort_plan(2 * n) if 2 * n <= (1 << 26) else plan
        sort_launches = 2 + 8 + 3 * plan["passes"] + 1             # memset, keys, gathers, passes, emit
        lookup_launches = 2 + 8 + 1 + 3 * (plan["passes"] + 1) + 2 + 7  # + member word and pass, 2 memsets, 7 kernels
        print(f"# 2^{logn}: tile {plan['tile']} workgroups {plan['groups']} (lookup {plan2['groups']}) passes {plan['passes']} "
              f"launches sort {sort_launches} lookup {lookup_launches} scratch sort {plan['sort_bytes']} "
              f"lookup {plan['lookup_bytes']}", flush=True)
        g = torch.Generator(device="cuda")
        g.manual_seed(logn)
        columns = {}
        table = amd.torch_u64((n, 4))
        amd.gen_scalars(table, 0x100C, montgomery=True)
        columns["full"] = (table[torch.randint(0, n, (n,), device="cuda", generator=g)].contiguous(), table)
        rng = torch.arange(n, device="cuda", dtype=torch.int64)
        columns["range16"] = (small(torch.randint(0, 1 << 16, (n,), device="cuda", generator=g)),
                              small(torch.where(rng < (1 << 16), rng, torch.zeros_like(rng))))
        other = amd.torch_u64((n, 4))
        amd.gen_scalars(other, 0x100D, montgomery=True)
        out, pin, ptab, tmp = (amd.torch_u64((n, 4)) for _ in range(4))
        for name, (inp, tab) in columns.items():
            legs = {"sort": lambda: amd.fr_sort(inp, out=out, is_async=True),
                    "lookup": lambda: amd.lookup_permute(inp, tab, count=False, out=(pin, ptab), is_async=True),
                    "mul": lambda: amd.vec_op("mul", inp, other, out=tmp, is_async=True)}
            # correctness once
            _, perm = amd.fr_sort(inp, out=out, perm=True)
            assert torch.equal(torch.sort(perm.long()).values, rng), "perm is a permutation"
            assert torch.equal(out, inp[perm.long()]), "sorted is input[perm]"
            std = amd.to_numpy_u64(amd.vec_op("scalar_mul", np.array([[1, 0, 0, 0]], dtype=np.uint64), out[:4096].contiguous(),
                                              out=amd.torch_u64((4096, 4))))  # x * 1 / R: the standard value
            keys = [int.from_bytes(row.tobytes(), "little") for row in std]
            assert keys == sorted(keys), "ascending by standard value"
            _, _, missing = amd.lookup_permute(inp, tab, out=(pin, ptab))
            assert missing == [0] and torch.equal(pin, out), "no missing value; A' is the sorted input"
            ts = {k: [] for k in legs}
            for rep in range(a.reps + 1):
                for k, fn in legs.items():
                    t = timed(fn)
                    if rep:
                        ts[k].append(t)
            med = {}
            line = f"lookup 2^{logn} {name}:"
            for k, v in ts.items():
                v.sort()
                med[k] = v[len(v) // 2]
                line += f" {k} median {med[k]:.3f} ms min {v[0]:.3f} max {v[-1]:.3f}"
            line += f" | sort / mul {med['sort'] / med['mul']:.1f}, lookup / mul {med['lookup'] / med['mul']:.1f}, " \
                    f"lookup / sort {med['lookup'] / med['sort']:.2f}"
            print(line, flush=True)
        del columns, table, other, out, pin, ptab, tmp


if __name__ == "__main__":
    main()
