#!/usr/bin/env python3
"""Point compression / decompression timing (device events, device-resident operands) at n = 2^16
and 2^20 valid points, both groups:

  candidates  decompress (mbls_g*_decompress): device records, device points and status, no count
              (a count is a host output and would make the call synchronous);
              compress (mbls_g*_compress): device points, device records
  comparator  check_points (mbls_g*_check_points) on the same points, device in, device status, no
              count: the same kind of work per lane (one fixed chain per point), from the same tree

The records are the compression of generated bases, and the decompression of those records is
compared with the bases once before the timing.  Valid records are the expensive input: a record
that fails an earlier test leaves before the chain.  One warm-up, then --reps timed rounds with the
legs interleaved in one process; prints median, min and max per leg and the decompress /
check_points ratio.  There is no pass / fail bound.  MBLS_LIB selects another in-tree build of the
library (the window-width variants of DESIGN.md 5.8)."""
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
    print(f"# {amd.lib().mbls_version().decode()} lib {os.path.relpath(amd.LIB_PATH, ROOT)} "
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
            amd.gen_bases(group, p, 0x5EED0051)
            rec = torch.zeros((n, 4 * nl), dtype=torch.uint8, device="cuda")
            amd.compress_points(group, p, out=rec)
            q = torch.zeros_like(p)
            status = torch.zeros((n,), dtype=torch.uint8, device="cuda")
            rec2 = torch.zeros_like(rec)
            _, _, bad = amd.decompress_points(group, rec, out=q, status=status)
            assert bad == 0 and not bool(status.any()) and torch.equal(p, q), "the round trip must be exact"

            legs = {"decompress": lambda: amd.decompress_points(group, rec, out=q, status=status, count=False,
                                                                is_async=True),
                    "compress": lambda: amd.compress_points(group, p, out=rec2, is_async=True),
                    "check": lambda: amd.check_points(group, p, out=status, count=False, is_async=True)}
            ts = {k: [] for k in legs}
            for rep in range(a.reps + 1):
                for k, fn in legs.items():
                    t = timed(fn)
                    if rep:
                        ts[k].append(t)
            assert torch.equal(rec, rec2) and torch.equal(p, q) and not bool(status.any())
            med = {}
            line = f"{group} serde 2^{logn}:"
            for k, v in ts.items():
                v.sort()
                med[k] = v[len(v) // 2]
                line += f" {k} median {med[k]:.3f} ms min {v[0]:.3f} max {v[-1]:.3f}"
            c = ts["check"]
            line += (f" | decompress / check {med['decompress'] / med['check']:.3f}, check spread "
                     f"{(c[-1] - c[0]) / med['check']:.3f}")
            print(line, flush=True)
            del p, q, rec, rec2, status


if __name__ == "__main__":
    main()
