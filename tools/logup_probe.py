#!/usr/bin/env python3
"""Log-derivative lookup timing (device events, device-resident operands) at size 2^20 and 2^22 with
K = 1 and K = 4 input columns:

  candidates   mult_uniform  mbls_fr_lookup_multiplicities, a 16-bit range table (table[j] = j mod 2^16,
                             standard form), input cells uniform over the range
               mult_equal    the same table, every input cell one value: the contention case
               prefix_sum    mbls_fr_prefix_sum, device total
               logup_sum     mbls_fr_logup_sum over random Montgomery columns, device total
  comparators  permute       mbls_fr_lookup_permute of the first input column and the same table
               add           bls12_381_vector_add at the same size: one addition per element
               composed      the terms from the element-wise entries: per column scalar_add_vec,
                             batch_inv, vector_add, for the table scalar_add_vec, batch_inv, vector_mul
                             by m, vector_sub (4 K + 3 passes, K + 1 Fermat chains per 64 elements)
               dict_cpu      the join as a single-threaded Python dictionary walk on the host, timed
                             once with time.perf_counter (operands already in host lists)

All from the same tree and process.  One warm-up, then --reps timed rounds with the legs
interleaved; prints median, min and max per leg and the ratios.  The results are checked once
before the timing: the counts against numpy.bincount, the running sum with vector_add on shifted
views, logup_sum against prefix_sum over the composed terms.  There is no pass / fail bound.
MBLS_LIB selects another in-tree build of the library."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE = 1 << 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--logn", type=int, nargs="*", default=[20, 22])
    ap.add_argument("--k", type=int, nargs="*", default=[1, 4])
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

    def small(v):
        w = np.zeros((len(v), 4), dtype=np.uint64)
        w[:, 0] = v
        return amd.torch_u64(w)

    for logn in a.logn:
        n = 1 << logn
        for K in a.k:
            rng = np.random.default_rng(logn * 10 + K)
            h_table = np.arange(n, dtype=np.uint64) & np.uint64(RANGE - 1)
            h_cells = [rng.integers(0, RANGE, size=n, dtype=np.uint64) for _ in range(K)]
            table, cells = small(h_table), [small(c) for c in h_cells]
            same = [small(np.full(n, 77, dtype=np.uint64)) for _ in range(K)]
            cols = [amd.torch_u64((n, 4)) for _ in range(K)]
            for c, col in enumerate(cols):
                amd.gen_scalars(col, 0x10C0 + c, montgomery=True)
            tab, mul, beta = amd.torch_u64((n, 4)), amd.torch_u64((n, 4)), amd.torch_u64((1, 4))
            amd.gen_scalars(tab, 0x10D0, montgomery=True)
            amd.gen_scalars(mul, 0x10D1, montgomery=True)
            amd.gen_scalars(beta, 0x10D2, montgomery=True)
            m, out, acc, tmp = (amd.torch_u64((n, 4)) for _ in range(4))
            pin, ptab = amd.torch_u64((n, 4)), amd.torch_u64((n, 4))
            tot = amd.torch_u64((1, 4))

            def composed():
                # batch_inv is synchronous by its own contract: the events still bracket the device work
                for c, col in enumerate(cols):
                    amd.vec_op("scalar_add", beta, col, out=tmp, is_async=True)
                    if c == 0:
                        amd.batch_inv(tmp, acc)
                    else:
                        amd.batch_inv(tmp, tmp)
                        amd.vec_op("add", acc, tmp, out=acc, is_async=True)
                amd.vec_op("scalar_add", beta, tab, out=tmp, is_async=True)
                amd.batch_inv(tmp, tmp)
                amd.vec_op("mul", mul, tmp, out=tmp, is_async=True)
                amd.vec_op("sub", acc, tmp, out=acc, is_async=True)

            legs = {"mult_uniform": lambda: amd.lookup_multiplicities(cells, table, "first", False, count=False, out=m,
                                                                      is_async=True),
                    "mult_equal": lambda: amd.lookup_multiplicities(same, table, "first", False, count=False, out=m,
                                                                    is_async=True),
                    "prefix_sum": lambda: amd.prefix_sum(cols[0], out=out, total=tot, is_async=True),
                    "logup_sum": lambda: amd.logup_sum(cols, tab, mul, beta, out=out, total=tot, is_async=True),
                    "permute": lambda: amd.lookup_permute(cells[0], table, mont=False, count=False, out=(pin, ptab),
                                                          is_async=True),
                    "add": lambda: amd.vec_op("add", cols[0], tab, out=tmp, is_async=True),
                    "composed": composed}

            # correctness once
            got, missing = amd.lookup_multiplicities(cells, table, "first", False)
            want = np.zeros(n, dtype=np.uint64)
            want[:RANGE] = sum(np.bincount(c.astype(np.int64), minlength=RANGE) for c in h_cells).astype(np.uint64)
            assert missing == [0] and np.array_equal(amd.to_numpy_u64(got)[:, 0], want), "counts equal numpy.bincount"
            got, missing = amd.lookup_multiplicities(same, table, "first", False)
            assert missing == [0] and int(amd.to_numpy_u64(got)[77, 0]) == K * n, "one row takes every cell"
            legs["prefix_sum"]()
            amd.vec_op("add", out, cols[0], out=tmp)
            assert torch.equal(tmp[:-1], out[1:]) and torch.equal(tmp[-1:], tot), "out[i+1] = out[i] + x[i]"
            composed()
            ref, rtot = amd.prefix_sum(acc, out=amd.torch_u64((n, 4)), total=True)
            legs["logup_sum"]()
            torch.cuda.synchronize()
            assert torch.equal(ref, out) and torch.equal(rtot, tot), "logup_sum equals prefix_sum of the composed terms"
            del ref, got

            # the host's dictionary walk, once
            t_list, c_lists = h_table.tolist(), [c.tolist() for c in h_cells]
            t0 = time.perf_counter()
            row = {}
            for j, v in enumerate(t_list):
                if v not in row:
                    row[v] = j
            counts, miss = [0] * n, 0
            for col in c_lists:
                for v in col:
                    j = row.get(v)
                    if j is None:
                        miss += 1
                    else:
                        counts[j] += 1
            dict_ms = (time.perf_counter() - t0) * 1e3
            assert miss == 0 and counts[:RANGE] == want[:RANGE].tolist()
            del t_list, c_lists, counts, row

            ts = {k: [] for k in legs}
            for rep in range(a.reps + 1):
                for k, fn in legs.items():
                    t = timed(fn)
                    if rep:
                        ts[k].append(t)
            med = {}
            line = f"logup 2^{logn} K {K}:"
            for k, v in ts.items():
                v.sort()
                med[k] = v[len(v) // 2]
                line += f" {k} median {med[k]:.3f} ms min {v[0]:.3f} max {v[-1]:.3f}"
            line += f" dict_cpu {dict_ms:.0f} ms (once)"
            ad = ts["add"]
            line += (f" | mult_uniform / permute {med['mult_uniform'] / med['permute']:.2f},"
                     f" mult_equal / mult_uniform {med['mult_equal'] / med['mult_uniform']:.2f},"
                     f" dict_cpu / mult_uniform {dict_ms / med['mult_uniform']:.0f},"
                     f" prefix_sum / add {med['prefix_sum'] / med['add']:.2f},"
                     f" logup_sum / composed {med['logup_sum'] / med['composed']:.2f},"
                     f" logup_sum / prefix_sum {med['logup_sum'] / med['prefix_sum']:.2f},"
                     f" add spread {(ad[-1] - ad[0]) / med['add']:.3f}")
            print(line, flush=True)
            del table, cells, same, cols, tab, mul, m, out, acc, tmp, pin, ptab


if __name__ == "__main__":
    main()
