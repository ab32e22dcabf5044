"""The binary-GCD inversion's sign corrections (csrc/mbls_binv.hpp), on the CPU: the Python model
(tests/binv_model.py) against pow(y, -1, m) and against the host harness's trace mode
(tests/binv_host.cpp, the header compiled with g++), the coverage condition on the fixture
tests/golden/binv_signs.json, and the negative control: model mutants of the correction that the
fixture catches in every cell and that the older inversion inputs of the GPU suite cannot catch.

The GPU side is tests/test_gpu_binv.py."""
import os
import random
import subprocess

import pytest

import binv_model as bm
import helpers as H
from helpers import pyref as pr
from test_gpu_field import FQ, FR, _inv_inputs

MODULI = {"fq": (pr.P, 12), "fr": (pr.R, 8)}


def load_cells():
    """{(field, row, when): [entry]} of the fixture, y as an integer"""
    cells = {}
    for c in H.load_golden("binv_signs.json")["cells"]:
        cells[(c["field"], c["row"], c["when"])] = [dict(e, y=int(e["y"], 16)) for e in c["entries"]]
    return cells


def fixture_values(field):
    return [e["y"] for (f, _, _), es in sorted(load_cells().items()) if f == field for e in es]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("binv") / "binv_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd", "csrc"),
                           os.path.join(H.ROOT, "tests", "binv_host.cpp"), "-o", str(exe)])

    def trace(field, ys):
        """[(inverse, steps, [(row, step)])] of the harness's trace mode"""
        w = MODULI[field][1]
        inp = "".join(f"{w} " + " ".join(f"{(y >> (32 * i)) & 0xffffffff:08x}" for i in range(w)) + "\n" for y in ys)
        out = subprocess.run([str(exe), "trace"], input=inp, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(ys)
        res = []
        for line in out:
            f = line.split()
            assert f[1] == "1"  # the four-lane form's roles agree
            res.append((sum(int(x, 16) << (32 * i) for i, x in enumerate(f[2:2 + w])), int(f[0]),
                        [(t[0], int(t[1:])) for t in f[2 + w:]]))
        return res
    return trace


def _edges(m):
    """the edge list of test_oracle.py::test_binary_gcd_inverse"""
    rnd = random.Random(7)
    vals = [1, 2, 3, m - 1, m - 2, (m + 1) // 2, 2 ** (m.bit_length() - 1)]
    vals += [rnd.randrange(1, 2 ** k) for k in range(1, m.bit_length(), 5)]
    vals += [m - rnd.randrange(1, 2 ** k) for k in range(1, m.bit_length(), 5)]
    return vals


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_model_against_pow_and_harness(harness, field):
    """value, outer steps and every correction's (row, step), on the fixture, the edge list and 300
    random values; and the events that every input meets are met"""
    m = MODULI[field][0]
    rnd = random.Random(0xB17 + len(field))
    ys = fixture_values(field) + _edges(m) + [rnd.randrange(1, m) for _ in range(300)]
    seen = set()
    for y, (hv, hsteps, hcorr) in zip(ys, harness(field, ys)):
        v, steps, trace = bm.inverse(y, m)
        assert v == pow(y, -1, m) == hv, hex(y)
        assert steps == hsteps and steps == len(trace) - 1, hex(y)
        assert bm.corrections(trace) == hcorr, hex(y)
        for t in trace[:-1]:
            seen |= {("clamped", t["clamped"]), ("xeq", t["xeq"])} | {("update",) + u for u in t["updates"]}
        seen.add(("final",) + trace[-1]["final"])
    assert {("clamped", True), ("clamped", False), ("xeq", True)} <= seen
    updates = {s[1:] for s in seen if s[0] == "update"}
    assert {neg for neg, _ in updates} == {False, True} and {subs for _, subs in updates} == {0, 1, 2}


def test_fixture_coverage_condition():
    """8 cells, 4 to 8 entries each, and every recorded (row, step, steps) is the model's trace: one
    correction, in that row, in outer step 1 (first) or after it (later)"""
    cells = load_cells()
    assert set(cells) == {(f, r, w) for f in MODULI for r in "ab" for w in ("first", "later")}
    for (field, row, when), entries in cells.items():
        m = MODULI[field][0]
        assert 4 <= len(entries) <= 8, (field, row, when)
        assert len({e["y"] for e in entries}) == len(entries)
        for e in entries:
            assert 0 < e["y"] < m
            v, steps, trace = bm.inverse(e["y"], m)
            assert v == pow(e["y"], -1, m)
            assert bm.corrections(trace) == [(e["row"], e["step"])] and steps == e["steps"], (field, hex(e["y"]))
            assert e["row"] == row and (e["step"] == 1) == (when == "first")
            assert e["step"] <= steps - 2  # no known input corrects in the last two outer steps


def mutant_catches(mutant):
    """{cell: entries for which the mutant's inverse is wrong}"""
    out = {}
    for (field, row, when), entries in load_cells().items():
        m = MODULI[field][0]
        out[(field, row, when)] = sum(bm.inverse(e["y"], m, mutant=mutant)[0] != pow(e["y"], -1, m) for e in entries)
    return out


@pytest.mark.parametrize("mutant", bm.MUTANTS)
def test_fixture_catches_the_mutant_in_every_cell(mutant):
    """a dropped correction, one applied to the wrong pipeline step and one taken from the wrong
    lane each return a wrong inverse for at least one entry of every cell they apply to (drop_a:
    the a cells, drop_b: the b cells, the others: all 8).  Measured, wrong inverses per cell of 8
    entries: drop_a 8 in each a cell and 0 in the b cells, drop_b 8 in each b cell and 0 in the a
    cells; early and lane0_for_both 8 in every cell except (fq | fr, a, first), where they are wrong
    for 4: the 4 random entries.  The 4 directed ones, y = m - (j << k) + e, end step 1 with
    f1 = 0, and with v = 0 after step 1 a wrong sign of u or of row 1 then never reaches v."""
    got = mutant_catches(mutant)
    for (field, row, when), wrong in got.items():
        if mutant in ("drop_a", "drop_b") and row != mutant[-1]:
            assert wrong == 0, (field, row, when)  # the mutant never fires there
        else:
            assert wrong >= 1, (field, row, when)


def test_old_inverse_inputs_catch_no_mutant():
    """the gap, stated as a test: on the 28 non-zero Fq inputs of test_gpu_field.py's inverse tests
    no correction happens, so every mutant returns the right inverse; the Fr list has 3 events"""
    xs = [x for x in _inv_inputs(FQ) if x]
    assert len(xs) == 28
    for x in xs:
        assert bm.corrections(bm.inverse(x, pr.P)[2]) == []
        for mutant in ("drop_a", "drop_b", "early"):
            assert bm.inverse(x, pr.P, mutant=mutant)[0] == pow(x, -1, pr.P), (mutant, hex(x))
    assert sum(bool(bm.corrections(bm.inverse(x, pr.R)[2])) for x in _inv_inputs(FR) if x) == 3
