#!/usr/bin/env python3
"""Regenerate tests/golden/binv_signs.json: inputs that steer the binary-GCD inversion
(csrc/mbls_binv.hpp) into its sign corrections.  Seeded and deterministic.

    python3 tests/golden/gen_binv_signs.py            # ~1 minute on 8 cores

A sign correction is `lincomb_shift(...) == true` in binv::inverse: the 64-bit approximations
ordered a and b the wrong way, f a + g b came out negative and the row is negated before it reaches
(u, v).  The fixture has 8 cells, field {fq, fr} x row {a, b} x step {first, later}, each with up to
8 raw integers y < m that have exactly one correction, in that row, in outer step 1 ("first") or in
a later one, with the recorded (row, step, steps).  The labels come from the host harness's trace
mode (tests/binv_host.cpp, built here with g++); tests/test_binv_model.py checks them against the
Python model.

Sources:
  first   y = m - (j << k) + e, k = 33, 36, .. < bitlen(m) - 34, j in {1, 3, 5, 0x1234567},
          e in {0, 2 j} (these end step 1 with f1 = 0, which hides a wrong sign of row 1), and
          up to 4 of the random values below whose one correction is in step 1
  later  (m +- 1) // j for j = 1 .. 297, and SEARCH random values per field from the harness's
          search mode (a splitmix64 stream per chunk)

What the last run found (it prints these figures; SEARCH = 3,000,000 random values per field):
  fq random    408 inversions with a correction (1 in 7,353): a first 12, a later 195, b first 3,
               b later 198; they take 17 (26 of them), 18 (331) or 19 (51) outer steps; the
               correction closest to the end is in step 15 of 17
  fr random    273 (1 in 10,989): a first 11, a later 140, b first 9, b later 113; 11 (7), 12 (222)
               or 13 (44) outer steps; closest to the end: step 10 of 12
  fq directed  726 of 840 candidates: 411 a first, 314 b first, 1 b later (step 9 of 16)
  fr directed  488 of 504: 244 a first, 244 b first
  (m +- 1)//j  fr 18 of 594: a first 2, a later 2, b first 2, b later 12; fq none
  In no family and in no random value: a correction in the last or in the second-to-last outer
  step, or two corrections in one inversion.  So there is no last-step cell: the final
  `lincomb_mod(nv, u, v, pf1, pg1)` after the loop has met a negated row for no known input, and
  the pending update of a correction is always issued inside the loop.
"""
import concurrent.futures
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
FIELDS = (("fq", P, 12), ("fr", R, 8))
SEARCH = 3_000_000
CHUNKS = 6
SEED = 0xB1A5
PER_CELL = 8


def build(tmp):
    exe = os.path.join(tmp, "binv_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "midnight-bls12-381-cuda_amd", "csrc"),
                           os.path.join(ROOT, "tests", "binv_host.cpp"), "-o", exe])
    return exe


def trace(exe, words, ys):
    """[(steps, [(row, step)])] of the harness's trace mode"""
    inp = "".join(f"{words} " + " ".join(f"{(y >> (32 * i)) & 0xffffffff:08x}" for i in range(words)) + "\n" for y in ys)
    out = subprocess.run([exe, "trace"], input=inp, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(ys)
    res = []
    for line in out:
        f = line.split()
        assert f[1] == "1"
        res.append((int(f[0]), [(t[0], int(t[1:])) for t in f[2 + words:]]))
    return res


def search(exe, words, seed, count):
    out = subprocess.run([exe, "search", str(words), str(seed), str(count)], capture_output=True, text=True, check=True)
    res = []
    for line in out.stdout.splitlines():
        f = line.split()
        res.append((int(f[0], 16), int(f[1]), [(t[0], int(t[1:])) for t in f[2:]]))
    return res


def spread(items, n):
    """n of the sorted items, evenly spaced, both ends included"""
    if len(items) <= n:
        return list(items)
    return [items[round(i * (len(items) - 1) / (n - 1))] for i in range(n)]


def main():
    cells = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for fi, (name, m, words) in enumerate(FIELDS):
            directed = [m - (j << k) + e for k in range(33, m.bit_length() - 34, 3) for j in (1, 3, 5, 0x1234567)
                        for e in (0, 2 * j)]
            small = [(m + s) // j for j in range(1, 298) for s in (-1, 1)]
            small = [y for y in small if 0 < y < m]
            found = {"directed": [(y, s, ev) for y, (s, ev) in zip(directed, trace(exe, words, directed)) if ev],
                     "small": [(y, s, ev) for y, (s, ev) in zip(small, trace(exe, words, small)) if ev]}
            with concurrent.futures.ThreadPoolExecutor(CHUNKS) as ex:
                jobs = [ex.submit(search, exe, words, SEED + 100 * fi + c, SEARCH // CHUNKS) for c in range(CHUNKS)]
                found["random"] = [r for j in jobs for r in j.result()]
            # the report that the docstring above records
            for src, rows in found.items():
                one = [(y, s, ev[0]) for y, s, ev in rows if len(ev) == 1]
                kinds = {}
                for y, s, (row, step) in one:
                    key = f"{row} {'first' if step == 1 else 'later'}"
                    kinds[key] = kinds.get(key, 0) + 1
                hist = {}
                for y, s, ev in rows:
                    hist[s] = hist.get(s, 0) + 1
                late = max(((step, s) for y, s, ev in rows for _, step in ev), key=lambda t: t[0] - t[1], default=None)
                print(f"{name} {src}: {len(rows)} with a correction, {len(rows) - len(one)} with more than one, "
                      f"{sorted(kinds.items())}, steps {sorted(hist.items())}, closest to the end (step, steps) {late}, "
                      f"in the last two steps {sum(1 for y, s, ev in rows for _, step in ev if step >= s - 1)}", file=sys.stderr)
            for row in "ab":
                # first: half random, half directed.  The directed family alone is degenerate: its
                # step 1 ends with f1 = 0, so a wrong sign of row 1 there changes nothing
                first = spread(sorted((y, s, ev[0]) for y, s, ev in found["random"] if ev == [(row, 1)]), PER_CELL // 2)
                first += spread(sorted((y, s, ev[0]) for y, s, ev in found["directed"] if ev == [(row, 1)]),
                                PER_CELL - len(first))
                later = sorted(((y, s, ev[0]) for src in ("small", "random") for y, s, ev in found[src]
                                if len(ev) == 1 and ev[0][0] == row and ev[0][1] > 1), key=lambda t: (t[2][1], t[0]))
                for when, cand in (("first", first), ("later", later)):
                    pick = spread(cand, PER_CELL)
                    assert len(pick) >= 4, (name, row, when)
                    cells.append({"field": name, "row": row, "when": when,
                                  "entries": [{"y": hex(y), "row": r, "step": step, "steps": s} for y, s, (r, step) in pick]})
    doc = {"about": "inputs of binv::inverse with one sign correction; written by tests/golden/gen_binv_signs.py",
           "cells": cells}
    with open(os.path.join(HERE, "binv_signs.json"), "w") as f:  # one entry per line
        f.write('{"about": %s,\n "cells": [\n' % json.dumps(doc["about"]))
        for i, c in enumerate(cells):
            head = {k: c[k] for k in ("field", "row", "when")}
            f.write("  " + json.dumps(head)[:-1] + ', "entries": [\n')
            f.write(",\n".join("   " + json.dumps(e) for e in c["entries"]))
            f.write("]}" + ("," if i + 1 < len(cells) else "") + "\n")
        f.write(" ]}\n")


if __name__ == "__main__":
    main()
