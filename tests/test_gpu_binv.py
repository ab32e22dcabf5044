"""The binary-GCD inversion (csrc/mbls_binv.hpp, mbls_binv_quad.hpp) steered into its sign
corrections on the device.

inv() / inv_quad() end every ICICLE-entry MSM (the one (x, y, 1) normalisation), every run of 8
points of projective_to_affine (and with it the EC-NTT's per-stage normalisation), the Fq2 / PFq2
inverses (the norm is inverted in Fq) and the G1 scalar-mul table normalisation.  Their only
data-dependent branches negate a row (f, g) when the 64-bit approximations ordered a and b the wrong
way; the negated row reaches (u, v) one outer step late, and in the quad form the flag crosses lanes
by DPP.  Random input takes those branches about once in 7,000 (Fq) or 11,000 (Fr) inversions, and
the 28 non-zero Fq inputs of test_gpu_field.py's inverse tests never do (3 of the Fr list's do), so
a dropped correction, one applied to the wrong row or pipeline step, or one read from the wrong
quad lane passed the whole suite.  Here every inversion layer runs on inputs that take the branch
(tests/golden/binv_signs.json), through the existing ops of tests/diag/libfield_diag.so and through
the public projective_to_affine entry points, and every result is compared exactly with Python
integers.

The fixture (tests/golden/gen_binv_signs.py writes it, tests/test_binv_model.py checks its labels
against the Python model tests/binv_model.py and the host harness): 8 cells, field {fq, fr} x
corrected row {a, b} x outer step {first, later}, 8 entries each, every entry with exactly one
correction.  The later cells span steps 2 .. 16 of 17-19 (fq) and 2 .. 10 of 11-13 (fr).

Model mutants, wrong inverses per cell of 8 entries (test_binv_model.py asserts >= 1): drop_a 8 in
each a cell; drop_b 8 in each b cell; early and lane0_for_both 8 in every cell except (fq | fr, a,
first), where 4: the directed entries y = m - (j << k) + e end step 1 with f1 = 0, which hides
them, the 4 random ones do not.  On the 28 older Fq inputs every mutant returns the right inverse.

Measured event rates, 3,000,000 random values per field (the generator prints them):
    fq  408 inversions with a correction (1 in 7,353): a first 12, a later 195, b first 3, b later 198
    fr  273 (1 in 10,989): a first 11, a later 140, b first 9, b later 113
    directed y = m - (j << k) + e: fq 725 of 840 in step 1 (411 a, 314 b), fr 488 of 504 (244 a, 244 b)
    (r +- 1) // j, j = 1 .. 297: fr 14 with a later-step correction, 4 with a first-step one
Reproduce: g++ -O2 -std=c++17 -I midnight-bls12-381-cuda_amd/csrc tests/binv_host.cpp -o binv_host;
`./binv_host search 12 0xB1A5 500000` (8 for Fr) prints one line per value with a correction, the
generator runs six such chunks per field (seeds 0xB1A5 + 100 field + chunk); `./binv_host trace`
labels the values given on standard input.

Never seen, in any family or random value: a correction in the last or second-to-last outer step
(the closest: step 16 of 18), two corrections in one inversion, a negative zero.  So the final
update after the loop has never met a negated row; the later cells reach as far as is known."""
import random

import numpy as np
import pytest

import binv_model as bm
from helpers import pyref as pr
from test_binv_model import load_cells
from test_gpu_field import FIELDS, FQ, PAIR, _f2_mont_inv, _f2_mont_mul, _inv_inputs, _minv, check, pair2, words
from test_gpu_field import run  # noqa: F401  (the probe fixture)

P = pr.P
LIMIT = 32  # cases per inversion launch (test_gpu_field.py: "at most 32 cases each")


def events(field):
    """the field's 32 fixture entries, cell by cell"""
    return [e for (f, _, _), es in sorted(load_cells().items()) if f == field for e in es]


def has_event(F, y, e=None):
    """the model's verdict on what the kernel is about to invert: e's correction (or any)"""
    c = bm.corrections(bm.inverse(y, F.m)[2])
    return c == [(e["row"], e["step"])] if e else bool(c)


def quiet_inputs(F):
    """32 inputs without a correction: the older list's (0 and the non-canonical zero m included,
    which return before the loop) and 1, 3 and powers of two, which leave the loop after anything
    from the fewest outer steps (13 for Fq, 9 for Fr) to the most (26, 17)"""
    g = random.Random(0xB0 + F.N)
    xs = [F.m, 1, 3] + [1 << k for k in range(28, F.m.bit_length() - 1, 46)] + [1 << (F.m.bit_length() - 2)]
    xs += [x for x in _inv_inputs(F) if not x or not has_event(F, x)]
    while len(xs) < 32:
        x = g.randrange(1, F.m)
        if not has_event(F, x):
            xs.append(x)
    xs = xs[:32]
    assert 0 in xs and F.m in xs
    steps = {bm.inverse(x, F.m)[1] for x in xs if x % F.m}
    assert len(steps) >= 6 and not any(has_event(F, x) for x in xs if x % F.m), sorted(steps)
    return xs


def launches(F):
    """[(name, inputs)]: event inputs only; event and quiet inputs alternating case by case (lane by
    lane for inv, quad by quad for inv_quad); and 19 cases, i.e. 64 + 12 lanes of the quad kernel:
    a second wave with one event quad, two quads that return before the loop, 13 exited quads"""
    ev = [e["y"] for e in events(F.name)]
    assert len(ev) == 32 and all(has_event(F, y) for y in ev)
    mixed = [x for pair in zip(ev, quiet_inputs(F)) for x in pair]
    assert len(ev) <= LIMIT
    return [("events", ev), ("alternating 0", mixed[:LIMIT]), ("alternating 1", mixed[LIMIT:]),
            ("trailing", ev[5::2][:12] + ev[:5] + [0, F.m])]


@pytest.mark.gpu
@pytest.mark.parametrize("field", ["fq", "fr"])
def test_inv_and_inv_quad_take_the_sign_corrections(run, field):  # noqa: F811
    F, base = FIELDS[field]
    for name, xs in launches(F):
        assert len(xs) <= LIMIT
        want = [_minv(F, x) for x in xs]
        tags = [{"tag": hex(x)} for x in xs]
        rows = [[x] for x in xs]
        check(words(run(base + 13, rows), 0, F.N), want, tags, f"inv, {name}")
        o = run(base + 15, rows)
        for lane in range(4):
            check(words(o, 12 * lane, F.N), want, tags, f"inv_quad lane {lane}, {name}")


# ---- Fq2: the norm is the event input
def fq2_with_norm(y, g):
    """(a0, a1), Montgomery words, with mont(a0, a0) + mont(a1, a1) == y; p = 3 mod 4"""
    while True:
        a1 = g.randrange(P)
        t = (y - FQ.mont(a1, a1)) * FQ.R % P
        a0 = pow(t, (P + 1) // 4, P)
        if a0 * a0 % P == t:
            assert (FQ.mont(a0, a0) + FQ.mont(a1, a1)) % P == y
            return (a0, a1)


def fq2_event_inputs():
    g = random.Random(0xF2B1)
    return [fq2_with_norm(e["y"], g) for e in events("fq")]


@pytest.mark.gpu
def test_fq2_inverses_with_an_event_norm(run):  # noqa: F811
    xs = fq2_event_inputs()
    assert len(xs) <= LIMIT
    for a, e in zip(xs, events("fq")):  # what the kernels will invert
        assert has_event(FQ, (FQ.mont(a[0], a[0]) + FQ.mont(a[1], a[1])) % P, e)
    rows = [[a[0], a[1]] for a in xs]
    tags = [{"tag": hex(e["y"])} for e in events("fq")]
    want = [_f2_mont_inv(a) for a in xs]
    check(pair2(run(32, rows), 0), want, tags, "Fq2 inv")
    q = run(38, rows)
    for lane in range(4):
        check(pair2(q, 24 * lane), want, tags, f"Fq2 inv_quad lane {lane}")
    check(pair2(run(PAIR + 6, rows), 0), want, tags, "PFq2 inv")


# ---- projective_to_affine: the run's prefix product of Z is the event input
RUN = 8  # points.hip P2A_RUN
# n -> its runs: True for an event run.  8: the only run; 17: the middle run and the final partial
# run; 64 + 1: first and middle runs beside quiet ones in the same wave, and a last run that holds
# the event point alone
PLANS = {8: [True], 17: [False, True, True], 65: [True, False, True, False, True, False, True, False, True]}


def _f2_plain_to_raw_quotient(target, prefix):
    """w with _f2_mont_mul(prefix, w) == target"""
    w = pr.f2_mul(target, pr.f2_inv(prefix))
    return (w[0] * FQ.R % P, w[1] * FQ.R % P)


def p2a_case(group, n, entries, seed):
    """(points, wanted affine points), Montgomery words: Jacobian triples (not on the curve: the
    kernel does not look) such that every event run's product of non-zero Z's, as the kernel forms
    it, is a fixture value (G2: has it as its norm); Z = 0 at two places inside a full event run"""
    g = random.Random(seed)
    g2 = group == "g2"
    rz = (lambda: (g.randrange(P), g.randrange(1, P))) if g2 else (lambda: g.randrange(1, P))
    one = (FQ.R % P, 0) if g2 else FQ.R % P
    zero = (0, 0) if g2 else 0
    mul = _f2_mont_mul if g2 else FQ.mont
    entries = iter(entries)
    pts, used = [], []
    for r, event in enumerate(PLANS[n]):
        size = min(RUN, n - RUN * r)
        zs = [rz() for _ in range(size)]
        if event:
            e = next(entries)
            used.append(e)
            if size == RUN:
                zs[2] = zs[5] = zero
            last = size - 1
            acc = one
            for z in zs[:last]:
                acc = mul(acc, z) if z != zero else acc
            if g2:
                target = fq2_with_norm(e["y"], g)
                zs[last] = _f2_plain_to_raw_quotient(target, acc)
            else:
                zs[last] = e["y"] * pow(acc, -1, P) * FQ.R % P
            assert zs[last] != zero
        acc = one  # the kernel's chain
        for z in zs:
            acc = mul(acc, z) if z != zero else acc
        inverted = (FQ.mont(acc[0], acc[0]) + FQ.mont(acc[1], acc[1])) % P if g2 else acc
        if event:
            assert inverted == e["y"] and has_event(FQ, inverted, e), (n, r)
        else:
            assert not has_event(FQ, inverted), (n, r)
        pts += [(rz(), rz(), z) for z in zs]
    assert len(pts) == n
    want = []
    for x, y, z in pts:
        if z == zero:
            want.append((zero, zero))
        elif g2:
            X, Y, Z = (tuple(pr.fq_from_mont(c) for c in v) for v in (x, y, z))
            zi = pr.f2_inv(Z)
            zi2 = pr.f2_mul(zi, zi)
            want.append(tuple(tuple(pr.fq_to_mont(c) for c in v) for v in (pr.f2_mul(X, zi2), pr.f2_mul(Y, pr.f2_mul(zi2, zi)))))
        else:
            X, Y, Z = (pr.fq_from_mont(v) for v in (x, y, z))
            zi = pow(Z, -1, P)
            want.append((pr.fq_to_mont(X * zi * zi % P), pr.fq_to_mont(Y * zi * zi * zi % P)))
    return pts, want, used


def _flat(group, coords):
    """u64 limbs of a tuple of field elements"""
    out = []
    for v in coords:
        for c in (v if group == "g2" else (v,)):
            out += pr.int_to_limbs(c, 6)
    return out


P2A_COMBOS = [("g1", "host"), ("g1", "device"), ("g2", "host"), ("g2", "device")]


def p2a_cases(group, where):
    """the three sizes of one (group, placement): 8 event runs, on 8 fixture entries of its own (one
    from each half cell), so that the four combinations use all 32"""
    k = P2A_COMBOS.index((group, where))
    mine = events("fq")[k::4]
    out, used = [], []
    for n in sorted(PLANS):
        pts, want, u = p2a_case(group, n, mine[len(used):], 0xA77 + 16 * k + n)
        out.append((n, pts, want))
        used += u
    assert used == mine and len(mine) == 8
    return out


def test_designed_inputs_have_the_event():
    """CPU: every designed input of this file passes its own conditions (they are asserted where the
    inputs are built): the Fq2 norms, the products of Z that projective_to_affine inverts, the
    quiet inputs' absence of an event, and the fixture's use: all 32 Fq entries by
    projective_to_affine"""
    for F in (FQ, FIELDS["fr"][0]):
        assert [len(xs) for _, xs in launches(F)] == [32, 32, 32, 19]
    assert len(fq2_event_inputs()) == 32
    seen = []
    for group, where in P2A_COMBOS:
        for n, pts, want in p2a_cases(group, where):
            assert len(pts) == len(want) == n
            seen += [z for _, _, z in pts]
    assert sum(z in (0, (0, 0)) for z in seen) == 4 * 2 * 6  # two Z = 0 in each full event run


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gpu_helpers
    gpu_helpers.amd.lib()
    return gpu_helpers.amd


@pytest.mark.gpu
@pytest.mark.parametrize("group,where", P2A_COMBOS)
def test_projective_to_affine_inverts_an_event_product(amd, group, where):
    import torch
    for n, pts, want in p2a_cases(group, where):
        jac = np.array([_flat(group, p) for p in pts], dtype=np.uint64)
        src = jac if where == "host" else amd.torch_u64(jac)
        out = None if where == "host" else torch.zeros((n, 12 if group == "g1" else 24), dtype=torch.int64, device="cuda")
        got = amd.convert_points(group, "to_affine", src, out=out)
        got = got if where == "host" else amd.to_numpy_u64(got)
        for i, w in enumerate(want):
            assert [int(v) for v in got[i]] == _flat(group, w), (n, i, "run", i // RUN)
