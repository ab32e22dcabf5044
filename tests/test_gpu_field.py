"""The saturated 32-bit-limb field arithmetic at its carry extremes.

csrc/mbls_rowfield.hpp (RFq / RFq2: carry-lookahead on 64-bit ballot masks), mbls_wavepoint.hpp
(one point operation per wave), mbls_pairfield.hpp (PFq2) and the scalar Fq / Fr / Fq2 of
mbls_field.hpp / mbls_fips.hpp are reached by the MSM / NTT parity tests only on random data: a
limb sum of 0xffffffff, a zero limb difference, t == p inside the reduction or a wave whose rows
take different sides of a wave-uniform branch never occur there.  Here every operation runs on
operands built for exactly those events (tests/field_cases.py), through tests/diag/libfield_diag.so
(the same headers, one operation per launch), and every result is compared with Python integers,
exactly.

CPU tests (no GPU): the ballot lookahead restated on Python / numpy 64-bit masks against a ripple
carry (exhaustive over the generate / propagate patterns of a row), a coverage condition on the
generated operands, and a negative control."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import field_cases as fc
import helpers as H
from helpers import pyref as pr

CSRC = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd", "csrc")
DIAG = os.path.join(H.ROOT, "tests", "diag", "libfield_diag.so")
FQ = fc.Field("fq", pr.P, 12)
FR = fc.Field("fr", pr.R, 8)
FIELDS = {"fq": (FQ, 0), "fr": (FR, 100)}  # field, probe op base
ROW, PAIR, WAVE = 200, 300, 400
M64 = (1 << 64) - 1
P = pr.P


# ----------------------------------------------------------------------------- the lookahead (CPU)
def _header_constants():
    src = open(os.path.join(CSRC, "mbls_rowfield.hpp")).read()
    lanes = int(re.search(r"RF_LIMB_LANES = (0x[0-9a-f]+)ull", src).group(1), 16)
    body = src[src.index("rf_reduce_once(uint32_t t)"):]
    top = [int(v, 16) for v in re.findall(r"(0x[0-9a-f]{16})ull", body[:body.index("return {t}")])]
    flag = src[src.index("row_top_flag(uint64_t B)"):]
    ones = int(re.search(r"& (0x[0-9a-f]{16})ull", flag).group(1), 16)
    shifts = [int(v) for v in re.search(r"\(B >> (\d+)\).*\n.*\(y << (\d+)\) - y", flag).groups()]
    return lanes, top, ones, shifts


def carries_in(G, Pm, lanes):
    """mbls_rowfield.hpp carries_in on 64-bit masks (Python ints or numpy uint64 arrays)"""
    Pm = Pm & lanes
    a = G | Pm
    return (a + G) ^ a ^ G


def row_top_flag(B, ones, shifts):
    y = (B >> shifts[0]) & ones
    return ((y << shifts[1]) - y) & M64


def test_header_mask_constants():
    lanes, top, ones, shifts = _header_constants()
    assert lanes == sum(0xfff << (16 * r) for r in range(4))  # limb lanes 0..11 of each row
    assert len(top) == 2 and top[0] == top[1] == sum(1 << (16 * r + 11) for r in range(4))  # limb 11 of each row
    assert ones == sum(1 << (16 * r) for r in range(4)) and shifts == [12, 16]


def _ripple_rows(G, Pm):
    """expected carry-in mask: per row a ripple over its 12 limb lanes (numpy uint64 arrays);
    lane 12 takes the carry out of limb 11, lanes 13..15 and lane 0 take none"""
    out = np.zeros_like(G)
    one = np.uint64(1)
    for r in range(4):
        c = np.zeros_like(G)
        for j in range(12):
            s = np.uint64(16 * r + j)
            out |= c << s
            c = ((G >> s) & one) | (((Pm >> s) & one) & c)
        out |= c << np.uint64(16 * r + 12)
    return out


def test_lookahead_matches_ripple_exhaustive():
    """all 3^12 generate / propagate / kill patterns of one row, in each of the four rows, the other
    rows random; again with the propagate bits of the pad lanes 12..15 set (a subtraction's pad
    lanes compare equal): they must not carry across a row boundary"""
    lanes = _header_constants()[0]
    n = 3 ** 12
    idx = np.arange(n, dtype=np.uint64)
    g16 = np.zeros(n, dtype=np.uint64)
    p16 = np.zeros(n, dtype=np.uint64)
    for j in range(12):
        d = (idx // np.uint64(3 ** j)) % np.uint64(3)
        g16 |= (d == 1).astype(np.uint64) << np.uint64(j)
        p16 |= (d == 2).astype(np.uint64) << np.uint64(j)
    rng = np.random.default_rng(0xCA221)
    pad_all = np.uint64(sum(0xf000 << (16 * r) for r in range(4)))
    for row in range(4):
        G = g16 << np.uint64(16 * row)
        Pm = p16 << np.uint64(16 * row)
        for q in range(4):
            if q == row:
                continue
            pq = rng.integers(0, 1 << 12, size=n, dtype=np.uint64)
            G |= (rng.integers(0, 1 << 12, size=n, dtype=np.uint64) & ~pq & np.uint64(0xfff)) << np.uint64(16 * q)
            Pm |= pq << np.uint64(16 * q)
        want = _ripple_rows(G, Pm)
        pads = (np.uint64(0), pad_all, rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) & pad_all)
        for pad in pads:
            got = carries_in(G, Pm | pad, np.uint64(lanes))
            assert np.array_equal(got, want), (row, "pad lanes" if np.any(pad) else "plain")
        if row < 3:  # the control: without the lane mask a full-row chain under set pad bits leaks
            leak = carries_in(G, Pm | pad_all, np.uint64(M64))
            assert not np.array_equal(leak, want)


def test_row_top_flag_bit_trick():
    _, _, ones, shifts = _header_constants()
    g = random.Random(5)
    for bits in range(16):
        for _ in range(8):
            B = g.getrandbits(64) & ~sum(1 << (16 * r + 12) for r in range(4))
            B |= sum(((bits >> r) & 1) << (16 * r + 12) for r in range(4))
            want = sum(0xffff << (16 * r) for r in range(4) if (bits >> r) & 1)  # row 3 included: the wrap
            assert row_top_flag(B, ones, shifts) == want, (bits, hex(B))


# ----------------------------------------------------------------------------- the generator (CPU)
STAGE_LIST = {"add": "add", "reduce": "add", "sub": "sub", "corr": "sub"}


@pytest.fixture(scope="module")
def lists():
    return {(F.name, k): fn(F) for F in (FQ, FR) for k, fn in (("add", fc.add_cases), ("sub", fc.sub_cases))}


def _runs(F, cases, stage, carry=1):
    got = set()
    for c in cases:
        if c["tag"] == "random" or (stage == "corr" and c["a"] >= c["b"]):
            continue
        G, Pb = fc.stage_gp(stage, F, c["a"], c["b"])
        got |= {(j, L) for j, L, cin in fc.live_runs(G, Pb) if cin == carry}
    return got


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_generator_coverage(lists, field):
    """a condition on the directed lists (random filler does not count): for the addition, the
    reduction, the subtraction and its + m correction a propagate run of every (start, length)
    under an entering carry / borrow; both sides of every wave-uniform branch; the exact-edge sums"""
    F = FIELDS[field][0]
    for stage, name in STAGE_LIST.items():
        missing = fc.wanted_runs(F) - _runs(F, lists[(field, name)], stage)
        assert not missing, (stage, sorted(missing))
    missing = fc.wanted_runs(F, with_carry=False) - _runs(F, lists[(field, "add")], "add", carry=0)
    assert not missing, ("add, no carry entering", sorted(missing))
    add = [c for c in lists[(field, "add")] if c["tag"] != "random"]
    sub = [c for c in lists[(field, "sub")] if c["tag"] != "random"]
    m, top = F.m, F.ml[-1]
    assert {c["cls"] for c in add} == {"early", "reduce"}  # rf_reduce_once's top-limb early-out
    assert {c["cls"] for c in sub} == {"borrow", "plain"}  # operator-'s `neg == 0`
    # behind the early-out: rows that subtract m and rows that keep t
    assert {c["a"] + c["b"] >= m for c in add if c["cls"] == "reduce"} == {True, False}
    sums = {c["a"] + c["b"] for c in add}
    assert {m - 1, m, m + 1, 2 * m - 2} <= sums
    eq_top = [s for s in sums if fc.limbs(s, F.N)[-1] == top]
    assert any(s > m for s in eq_top) and any(s < m for s in eq_top)
    assert all(0 <= c["a"] < m and 0 <= c["b"] < m for c in lists[(field, "add")] + lists[(field, "sub")])
    # subtraction edges
    assert any(c["a"] == c["b"] for c in sub) and any(c["a"] == c["b"] - 1 for c in sub)
    assert {c["b"] for c in sub if c["a"] == 0} >= {0, 1, m - 1}
    # a borrow through all limbs: limb 0 borrows, every other limb is equal
    assert any(fc.stage_gp("sub", F, c["a"], c["b"]) == ([1] + [0] * (F.N - 1), [0] + [1] * (F.N - 1)) for c in sub)


def _wave_masks(stage, cases):
    """the 64-bit generate / propagate ballots of a wave whose rows hold up to 4 Fq cases, pad lanes
    as the device sees them: a subtraction's / reduction's pad lanes compare equal (0 == 0), the
    correction's lane 12 holds 0xffffffff after a borrow"""
    G = Pm = 0
    for r, c in enumerate(cases):
        g, p = fc.stage_gp(stage, FQ, c["a"], c["b"])
        pad = {"add": 0, "sub": 0xf, "reduce": 0xf, "corr": 1 if c["a"] < c["b"] else 0}[stage]
        G |= sum(b << j for j, b in enumerate(g)) << (16 * r)
        Pm |= (sum(b << j for j, b in enumerate(p)) | (pad << 12)) << (16 * r)
    return G, Pm


def _wave_want(stage, cases):
    want = 0
    for r, c in enumerate(cases):
        cin = fc.ripple(*fc.stage_gp(stage, FQ, c["a"], c["b"]))
        want |= sum(b << j for j, b in enumerate(cin)) << (16 * r)
    return want


def _cut_model(G, Pm, lanes):
    """a broken lookahead: a propagate chain cut at length 1"""
    Pm &= lanes
    return ((G | (Pm & (G << 1))) << 1) & M64


def test_lookahead_on_generated_cases_and_negative_control(lists):
    """the header's lookahead agrees with the ripple carry on every wave of the generated Fq lists (in
    the grouped and the interleaved order); with RF_LIMB_LANES all ones, or with a chain cut at
    length 1, it does not: the cases would catch those bugs"""
    lanes = _header_constants()[0]
    for stage, name in STAGE_LIST.items():
        cases = lists[("fq", name)]
        bad_lanes = bad_cut = 0
        for order in (fc.grouped(cases), fc.interleaved(cases)):
            for k in range(0, len(order), 4):
                wave = [cases[i] for i in order[k:k + 4]]
                G, Pm = _wave_masks(stage, wave)
                want = _wave_want(stage, wave)
                assert carries_in(G, Pm, lanes) & M64 == want, (stage, k)
                bad_lanes += carries_in(G, Pm, M64) & M64 != want
                bad_cut += _cut_model(G, Pm, lanes) != want
        assert bad_cut > 0, stage
        if stage != "add":  # an addition's pad lanes never propagate (0 + 0)
            assert bad_lanes > 0, stage


# ----------------------------------------------------------------------------- the probe (GPU)
@pytest.fixture(scope="module")
def run():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    if not os.path.exists(DIAG):
        pytest.fail(f"{DIAG} not built (__graft_entry__.build())")
    L = ctypes.CDLL(DIAG)
    L.field_diag_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.field_diag_run.restype = ctypes.c_int
    iw, ow = L.field_diag_in_words(), L.field_diag_out_words()

    failed = []

    def go(op, rows):
        """rows: per case a list of operands (integers below 2^384, one 12-word slot each)"""
        if failed:  # a launch that failed leaves the device in doubt: nothing more runs on it
            pytest.fail(f"the probe failed earlier (op {failed[0][0]}: {failed[0][1]})")
        a = np.zeros((len(rows), iw), dtype=np.uint32)
        for i, ops in enumerate(rows):
            for k, v in enumerate(ops):
                a[i, 12 * k:12 * k + 12] = np.frombuffer(int(v).to_bytes(48, "little"), dtype="<u4")
        o = np.zeros((len(rows), ow), dtype=np.uint32)
        rc = L.field_diag_run(op, a.ctypes.data, o.ctypes.data, len(rows))
        if rc != 0:
            failed.append((op, rc))
        assert rc == 0, (op, rc)
        return o
    return go


def words(o, start, n=12):
    """integers of the n words at `start` of every case"""
    return [fc.val(r[start:start + n]) for r in o.astype(object)]


def row_vals(o, elem=0):
    """a row result: 16 words per element, the pad lanes 12..15 zero"""
    assert not o[:, 16 * elem + 12:16 * elem + 16].any(), "pad lanes not zero"
    return words(o, 16 * elem)


def row_flags(o):
    assert (o[:, :16] == o[:, :1]).all(), "a row predicate is not row-uniform"
    return [int(v) for v in o[:, 0]]


def run_orders(run, op, cases, rows):
    """one launch in the list's order, then grouped by class (all rows of a wave on one side of each
    wave-uniform branch), interleaved (mixed waves), and with n % 4 = 1, 2, 3 (a last wave with
    exited rows): per-case outputs identical across all of them"""
    base = run(op, rows)
    n = len(rows)
    for name, order in (("grouped", fc.grouped(cases)), ("interleaved", fc.interleaved(cases))):
        o = run(op, [rows[i] for i in order])
        bad = np.nonzero((o != base[order]).any(axis=1))[0]
        assert bad.size == 0, (op, name, [cases[order[i]]["tag"] for i in bad[:4]])
        cut = len(order) - 1  # and a mixed last wave with exited rows
        assert np.array_equal(run(op, [rows[i] for i in order[:cut]]), base[order[:cut]]), (op, name, "cut")
    for k in (1, 2, 3):
        cut = n - ((n - k) % 4)
        if cut > 0:
            assert cut % 4 == k
            assert np.array_equal(run(op, rows[:cut]), base[:cut]), (op, "n % 4", k)
    return base


def check(got, want, cases, what):
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (what, len(bad), [(cases[i].get("tag"), hex(got[i]), hex(want[i])) for i in bad[:3]])


# ---- additions and subtractions
@pytest.mark.gpu
@pytest.mark.parametrize("field", ["fq", "fr"])
def test_scalar_add_sub(run, lists, field):
    F, base = FIELDS[field]
    m, n = F.m, F.N
    add, sub = lists[(field, "add")], lists[(field, "sub")]
    rows = [[c["a"], c["b"]] for c in add]
    check(words(run(base + 0, rows), 0, n), [(c["a"] + c["b"]) % m for c in add], add, "+")
    check(words(run(base + 3, rows), 0, n), [2 * c["a"] % m for c in add], add, "dbl")
    rows = [[c["a"], c["b"]] for c in sub]
    check(words(run(base + 1, rows), 0, n), [(c["a"] - c["b"]) % m for c in sub], sub, "-")
    check(words(run(base + 2, rows), 0, n), [-c["a"] % m for c in sub], sub, "neg")
    if field == "fq":  # the raw sum: exactly a + b
        check(words(run(20, [[c["a"], c["b"]] for c in add]), 0), [c["a"] + c["b"] for c in add], add, "add_in")


@pytest.mark.gpu
def test_row_add_sub_against_integers_and_scalar(run, lists):
    add, sub = lists[("fq", "add")], lists[("fq", "sub")]
    ra = [[c["a"], c["b"]] for c in add]
    rs = [[c["a"], c["b"]] for c in sub]
    o = run_orders(run, ROW + 0, add, ra)
    check(row_vals(o), [(c["a"] + c["b"]) % P for c in add], add, "row +")
    assert np.array_equal(o[:, :12], run(0, ra)[:, :12]), "row + vs scalar +"
    check(row_vals(run_orders(run, ROW + 3, add, ra)), [2 * c["a"] % P for c in add], add, "row dbl")
    check(row_vals(run_orders(run, ROW + 6, add, ra)), [c["a"] + c["b"] for c in add], add, "row add_in")
    o = run_orders(run, ROW + 1, sub, rs)
    check(row_vals(o), [(c["a"] - c["b"]) % P for c in sub], sub, "row -")
    assert np.array_equal(o[:, :12], run(1, rs)[:, :12]), "row - vs scalar -"
    check(row_vals(run_orders(run, ROW + 2, sub, rs)), [-c["a"] % P for c in sub], sub, "row neg")
    # the sub list taken as b - a: the other side of every branch
    rb = [[c["b"], c["a"]] for c in sub]
    swapped = [dict(c, cls="borrow" if c["b"] < c["a"] else "plain") for c in sub]
    check(row_vals(run_orders(run, ROW + 1, swapped, rb)), [(c["b"] - c["a"]) % P for c in sub], sub, "row b - a")


# ---- products
@pytest.fixture(scope="module")
def muls():
    return {F.name: (fc.mul_cases(F), fc.sqr_cases(F)) for F in (FQ, FR)}


@pytest.mark.gpu
@pytest.mark.parametrize("field", ["fq", "fr"])
def test_scalar_products(run, muls, field):
    F, base = FIELDS[field]
    m, n = F.m, F.N
    mc, sc = muls[field]
    rows = [[c["a"], c["b"]] for c in mc]
    want = [F.mont(c["a"], c["b"]) for c in mc]
    check(words(run(base + 4, rows), 0, n), want, mc, "operator*")
    check(words(run(base + 5, rows), 0, n), want, mc, "mul_cios")
    check(words(run(base + 6, [[c["a"]] for c in sc]), 0, n), [F.mont(c["a"], c["a"]) for c in sc], sc, "sqr")
    check(words(run(base + 11, [[c["a"]] for c in sc]), 0, n), [c["a"] * F.R % m for c in sc], sc, "to_mont")
    check(words(run(base + 12, [[c["a"]] for c in sc]), 0, n), [c["a"] * F.Rinv % m for c in sc], sc, "from_mont")
    # RED = false: a up to 2m - 1 against a canonical b: congruent and < 2m
    lazy = [dict(c, a=c["a"] + (m if i % 2 else 0)) for i, c in enumerate(mc)]
    lazy += [{"a": 2 * m - 1, "b": b, "tag": "2m-1"} for b in (m - 1, 1, 0, F.R % m)]
    for op, rows, ref in ((7, [[c["a"], c["b"]] for c in lazy], [F.mont(c["a"], c["b"]) for c in lazy]),
                          (8, [[c["a"]] for c in sc], [F.mont(c["a"], c["a"]) for c in sc])):
        got = words(run(base + op, rows), 0, n)
        assert all(g < 2 * m for g in got), ("RED=false bound", op)
        check([g % m for g in got], ref, lazy if op == 7 else sc, f"RED=false op {op}")
    # mul2: a b + c d with one reduction
    S = fc.specials(F)
    g = random.Random(0x22)
    quads = [(m - 1,) * 4] + [(S[i % len(S)], S[(i // 3) % len(S)], S[(i * 5 + 1) % len(S)], S[(i // 7 + 2) % len(S)])
                              for i in range(120)] + [tuple(g.randrange(m) for _ in range(4)) for _ in range(64)]
    ref = [(a * b + c * d) * F.Rinv % m for a, b, c, d in quads]
    tags = [{"tag": str(i)} for i in range(len(quads))]
    check(words(run(base + 9, [list(q) for q in quads]), 0, n), ref, tags, "mul2")
    got = words(run(base + 10, [list(q) for q in quads]), 0, n)
    assert all(v < 2 * m for v in got)
    check([v % m for v in got], ref, tags, "mul2 RED=false")


def _raw_cases():
    """operands of the Fq raw forms at their stated maxima"""
    g = random.Random(0x1A)
    S = fc.specials(FQ)
    vals = S + [g.randrange(P) for _ in range(16)]
    return vals, [(a, b) for a in (P - 1, P - 2, 0, 1) for b in S] + [(g.randrange(P), g.randrange(P)) for _ in range(32)]


@pytest.mark.gpu
def test_fq_raw_forms_scalar_and_row(run, muls):
    vals, pairs = _raw_cases()
    sc = muls["fq"][1]
    ops1 = [[c["a"], P - 1] for c in sc]  # the next slot is not zero: a row's pad lanes must not load it
    # raw: exact integers, no reduction; row pad lanes stay zero (row_vals)
    for k, (sop, rop) in ((1, (21, ROW + 7)), (2, (22, ROW + 8)), (3, (None, ROW + 9))):
        want = [c["a"] << k for c in sc]
        if sop is not None:
            check(words(run(sop, ops1), 0), want, sc, f"x{1 << k}_in")
        check(row_vals(run_orders(run, rop, sc, ops1)), want, sc, f"row x{1 << k}_in")
    check(words(run(23, ops1), 0), [P - c["a"] for c in sc], sc, "neg_in")
    assert words(run(23, [[0], [P - 1]]), 0) == [P, 1]
    # fed into a product: x2 / x4 / x8 (rows) of up to m - 1 against a canonical partner
    tags = [{"tag": f"{hex(a)[:12]} {hex(b)[:12]}", "cls": "lo" if i % 2 else "hi"} for i, (a, b) in enumerate(pairs)]
    rows = [[a, b] for a, b in pairs]
    for k, sop, rop in ((1, 25, ROW + 11), (2, 26, ROW + 12), (3, None, ROW + 13)):
        want = [FQ.mont(a << k, b) for a, b in pairs]
        o = run_orders(run, rop, tags, rows)
        check(row_vals(o), want, tags, f"row x{1 << k}_in product")
        if sop is not None:
            s = run(sop, rows)
            check(words(s, 0), want, tags, f"x{1 << k}_in product")
            assert np.array_equal(s[:, :12], o[:, :12])
    check(words(run(27, rows), 0), [FQ.mont(P - a, b) for a, b in pairs], tags, "neg_in product")
    # add_in: a sum of two against a canonical partner; sums of three (up to 3p - 3) squared, and
    # two such sums multiplied (scalar: "two operands up to 3p")
    tri = [(P - 1, P - 1, P - 1), (P - 1, P - 1, 0), (0, 0, 0), (P - 1, 1, 0)] + \
          [(vals[i % len(vals)], vals[(i * 3 + 1) % len(vals)], vals[(i * 7 + 2) % len(vals)]) for i in range(40)]
    ttag = [{"tag": str(i), "cls": "ab"[i % 2]} for i in range(len(tri))]
    rows = [list(t) for t in tri]
    want = [FQ.mont(a + b, c) for a, b, c in tri]
    o = run_orders(run, ROW + 10, ttag, rows)
    check(row_vals(o), want, ttag, "row add_in product")
    check(words(run(24, rows), 0), want, ttag, "add_in product")
    want = [FQ.mont(a + b + c, a + b + c) for a, b, c in tri]
    check(words(run(28, rows), 0), want, ttag, "sqr of a 3-sum")
    check(row_vals(run_orders(run, ROW + 19, ttag, rows)), want, ttag, "row sqr of a 3-sum")
    rows6 = [list(tri[i]) + list(tri[(i * 5 + 3) % len(tri)]) for i in range(len(tri))]
    check(words(run(29, rows6), 0), [FQ.mont(sum(r[:3]), sum(r[3:])) for r in rows6], ttag, "3-sum x 3-sum")


@pytest.mark.gpu
def test_row_products_against_integers_and_scalar(run, muls):
    mc, sc = muls["fq"]
    rows = [[c["a"], c["b"]] for c in mc]
    o = run_orders(run, ROW + 4, mc, rows)
    check(row_vals(o), [FQ.mont(c["a"], c["b"]) for c in mc], mc, "row *")
    assert np.array_equal(o[:, :12], run(4, rows)[:, :12]), "row * vs scalar *"
    r1 = [[c["a"]] for c in sc]
    check(row_vals(run_orders(run, ROW + 5, sc, r1)), [FQ.mont(c["a"], c["a"]) for c in sc], sc, "row sqr")
    check(row_vals(run_orders(run, ROW + 14, sc, r1)), [c["a"] * FQ.Rinv % P for c in sc], sc, "row from_mont")
    check(row_vals(run_orders(run, ROW + 20, sc, r1)), [c["a"] * FQ.R % P for c in sc], sc, "row a * r2()")
    # rf_load / rf_store round trip
    o = run_orders(run, ROW + 18, sc, [[c["a"], P - 1] for c in sc])
    assert words(o, 0) == [c["a"] for c in sc] and not o[:, 12:].any()


def row_product_overflow_cases():
    """regression: the row product's round added the whole redundant limb t_j (up to 3 (2^32 - 1)) to
    a_j b_i in one 64-bit register; with a_j = b_i = 0xffffffff and t_j >= 2^33 - 1 the sum passed
    2^64 and the product came out wrong (found by `ones[0:2] x ones[0:2]`: a = b = 2^64 - 1).  Both
    operands need an all-ones limb, and t_j has to be large when they meet"""
    ones = lambda j, L: ((1 << (32 * L)) - 1) << (32 * j)  # noqa: E731
    pairs = [(ones(0, 2), ones(0, 2)), (ones(0, 11), ones(0, 11)), (ones(3, 4), ones(0, 11)), (ones(10, 1), ones(9, 2)),
             (ones(0, 11) + (1 << 352), ones(0, 11)), ((P >> 1) | ones(4, 2), ones(0, 11))]
    return [{"a": a, "b": b, "tag": f"overflow regression {i}", "cls": "ab"[i % 2]} for i, (a, b) in enumerate(pairs)]


@pytest.mark.gpu
def test_row_product_all_ones_limbs_regression(run):
    cases = row_product_overflow_cases()
    assert all(0 <= c["a"] < P and 0 <= c["b"] < P for c in cases)
    rows = [[c["a"], c["b"]] for c in cases]
    want = [FQ.mont(c["a"], c["b"]) for c in cases]
    check(row_vals(run_orders(run, ROW + 4, cases, rows)), want, cases, "row *")
    check(row_vals(run(ROW + 5, rows)), [FQ.mont(c["a"], c["a"]) for c in cases], cases, "row sqr")
    # the unreduced operand forms meet the same round
    check(row_vals(run(ROW + 13, rows)), [FQ.mont(8 * c["a"], c["b"]) for c in cases], cases, "row x8_in product")


# ---- inverses (at most 32 cases each)
def _inv_inputs(F):
    g = random.Random(0x1F ^ F.N)
    return fc.specials(F) + [g.randrange(1, F.m) for _ in range(29 - len(fc.specials(F)))]


def _minv(F, x):
    """Montgomery-form inverse: x = a R -> a^-1 R; 0 -> 0 (inv / inv_fermat: "0 -> 0")"""
    return pow(x, -1, F.m) * F.R * F.R % F.m if x % F.m else 0


@pytest.mark.gpu
@pytest.mark.parametrize("field", ["fq", "fr"])
def test_scalar_inverses(run, field):
    F, base = FIELDS[field]
    xs = _inv_inputs(F)
    assert len(xs) <= 32 and 0 in xs
    want = [_minv(F, x) for x in xs]
    tags = [{"tag": hex(x)[:14]} for x in xs]
    rows = [[x] for x in xs]
    check(words(run(base + 13, rows), 0, F.N), want, tags, "inv")
    check(words(run(base + 14, rows), 0, F.N), want, tags, "inv_fermat")
    # inv / inv_quad reduce their input once: the non-canonical zero m is a valid input -> 0
    assert words(run(base + 13, [[F.m], [F.m + 1]]), 0, F.N) == [0, _minv(F, 1)]
    o = run(base + 15, rows + [[F.m]])
    for lane in range(4):  # every lane of the quad holds the result
        check(words(o, 12 * lane, F.N), want + [0], tags + [{"tag": "m"}], f"inv_quad lane {lane}")
    # a quad launch with exited trailing quads: 3 cases = 12 of 64 lanes
    assert np.array_equal(run(base + 15, rows[:3]), o[:3])


def _f2(a):
    return (a[0] % P, a[1] % P)


def _f2_mont_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) * FQ.Rinv % P, (a[0] * b[1] + a[1] * b[0]) * FQ.Rinv % P)


def _f2_mont_inv(a):
    if a == (0, 0):
        return (0, 0)  # the norm's inverse is inv(0) = 0
    ni = _minv(FQ, (FQ.mont(a[0], a[0]) + FQ.mont(a[1], a[1])) % P)
    return (FQ.mont(a[0], ni), -FQ.mont(a[1], ni) % P)


def _f2_inv_inputs():
    g = random.Random(0x2F)
    S = fc.specials(FQ)
    xs = [(0, 0), (1, 0), (0, 1), (P - 1, P - 1), (0, P - 1), (FQ.R % P, 0)]
    xs += [(S[i % len(S)], S[(i * 3 + 2) % len(S)]) for i in range(10)]
    return xs + [(g.randrange(P), g.randrange(P)) for _ in range(32 - len(xs))]


def pair2(o, start, stride=12):
    return list(zip(words(o, start), words(o, start + stride)))


@pytest.mark.gpu
def test_fq2_all_layers(run):
    """Fq2 +, -, *, sqr, predicates: the scalar Fq2, the row RFq2 and the pair PFq2 against Python
    integers and word for word against each other; PFq2 neg / dbl / one()"""
    cases = fc.fq2_cases(FQ)
    rows = [[c["a"][0], c["a"][1], c["b"][0], c["b"][1]] for c in cases]
    ref = {
        "+": [_f2((c["a"][0] + c["b"][0], c["a"][1] + c["b"][1])) for c in cases],
        "-": [_f2((c["a"][0] - c["b"][0], c["a"][1] - c["b"][1])) for c in cases],
        "*": [_f2_mont_mul(c["a"], c["b"]) for c in cases],
        "sqr": [_f2_mont_mul(c["a"], c["a"]) for c in cases],
    }
    for name, sop, rop, pop in (("+", 33, ROW + 30, PAIR + 0), ("-", 34, ROW + 31, PAIR + 1), ("*", 30, ROW + 32, PAIR + 4),
                                ("sqr", 31, ROW + 33, PAIR + 5)):
        s = run(sop, rows)
        r = run_orders(run, rop, cases, rows)
        p = run_orders(run, pop, cases, rows)
        check(pair2(s, 0), ref[name], cases, "Fq2 " + name)
        assert not r[:, 12:16].any() and not r[:, 28:32].any(), "pad lanes"
        assert np.array_equal(s[:, :24], p[:, :24]), ("pair vs scalar", name)
        assert np.array_equal(s[:, :12], r[:, :12]) and np.array_equal(s[:, 12:24], r[:, 16:28]), ("row vs scalar", name)
    # the product-sum exactly as PFq2::operator* forms it (neg_in partner), on the scalar mul2
    check(pair2(run(37, rows), 0), ref["*"], cases, "mul2 with the neg_in partner")
    for name, rop, pop, k in (("neg", ROW + 37, PAIR + 2, -1), ("dbl", ROW + 38, PAIR + 3, 2)):
        want = [_f2((k * c["a"][0], k * c["a"][1])) for c in cases]
        check(pair2(run_orders(run, pop, cases, rows), 0), want, cases, "pair " + name)
        r = run_orders(run, rop, cases, rows)
        check(list(zip(row_vals(r, 0), row_vals(r, 1))), want, cases, "row Fq2 " + name)
    assert pair2(run(PAIR + 9, rows[:3]), 0) == [(FQ.R % P, 0)] * 3


@pytest.mark.gpu
def test_fq2_inverses_all_layers(run):
    xs = _f2_inv_inputs()
    assert len(xs) <= 32
    rows = [[a[0], a[1]] for a in xs]
    tags = [{"tag": str(i), "cls": "ab"[i % 2]} for i in range(len(xs))]
    want = [_f2_mont_inv(a) for a in xs]
    s = run(32, rows)
    check(pair2(s, 0), want, tags, "Fq2 inv")
    q = run(38, rows)
    for lane in range(4):
        assert np.array_equal(q[:, 24 * lane:24 * lane + 24], s[:, :24]), ("Fq2 inv_quad lane", lane)
    r = run_orders(run, ROW + 34, tags, rows)
    check(list(zip(row_vals(r, 0), row_vals(r, 1))), want, tags, "RFq2 inv")
    p = run_orders(run, PAIR + 6, tags, rows)
    assert np.array_equal(p[:, :24], s[:, :24]), "PFq2 inv vs Fq2 inv"


@pytest.mark.gpu
def test_row_inverse(run):
    xs = _inv_inputs(FQ)
    tags = [{"tag": hex(x)[:14], "cls": "ab"[i % 2]} for i, x in enumerate(xs)]
    o = run_orders(run, ROW + 15, tags, [[x] for x in xs])
    check(row_vals(o), [_minv(FQ, x) for x in xs], tags, "row inv")  # Fermat: 0 -> 0


# ---- predicates
@pytest.mark.gpu
def test_predicates_all_layers(run):
    pc = fc.predicate_cases(FQ)
    rows = [[c["a"], c["b"]] for c in pc]
    zero = [int(c["a"] == 0) for c in pc]
    eq = [int(c["a"] == c["b"]) for c in pc]
    assert [int(v) for v in run(16, rows)[:, 0]] == zero and [int(v) for v in run(17, rows)[:, 0]] == eq
    assert row_flags(run_orders(run, ROW + 16, pc, rows)) == zero
    assert row_flags(run_orders(run, ROW + 17, pc, rows)) == eq
    fr = fc.predicate_cases(FR)
    rr = [[c["a"], c["b"]] for c in fr]
    assert [int(v) for v in run(116, rr)[:, 0]] == [int(c["a"] == 0) for c in fr]
    assert [int(v) for v in run(117, rr)[:, 0]] == [int(c["a"] == c["b"]) for c in fr]
    # Fq2: zero / equal in one component only, and every one-limb difference in either component
    c2, r2 = [], []
    for c in pc:
        for comp in (0, 1):
            a = (c["a"], 0) if comp == 0 else (0, c["a"])
            b = (c["b"], 0) if comp == 0 else (0, c["b"])
            c2.append({"a": a, "b": b, "tag": c["tag"], "cls": c["cls"] + str(comp)})
    v = 0x1234567 << 200
    c2 += [{"a": (v, 0), "b": (v, v), "tag": "c0 equal only", "cls": "ne0"},
           {"a": (0, v), "b": (v, v), "tag": "c1 equal only", "cls": "ne1"},
           {"a": (v, v), "b": (v, v), "tag": "equal", "cls": "eq0"}]
    r2 = [[c["a"][0], c["a"][1], c["b"][0], c["b"][1]] for c in c2]
    zero = [int(c["a"] == (0, 0)) for c in c2]
    eq = [int(c["a"] == c["b"]) for c in c2]
    assert [int(x) for x in run(35, r2)[:, 0]] == zero and [int(x) for x in run(36, r2)[:, 0]] == eq
    assert row_flags(run_orders(run, ROW + 35, c2, r2)) == zero
    assert row_flags(run_orders(run, ROW + 36, c2, r2)) == eq
    for op, want in ((PAIR + 7, zero), (PAIR + 8, eq)):
        o = run_orders(run, op, c2, r2)
        assert [int(x) for x in o[:, 0]] == want and [int(x) for x in o[:, 1]] == want  # both lanes of the pair


# ---- wave formulas
def _jac(group, pt, z):
    """affine pt (None: infinity) as Montgomery Jacobian coordinates with the given Z (Fq ints, flat)"""
    if group == "g1":
        if pt is None:
            x, y, z = z, (z * 5 + 1) % P, 0  # Z = 0 with arbitrary X, Y
        else:
            x, y = pt[0] * z * z % P, pt[1] * z * z * z % P
        return [pr.fq_to_mont(v) for v in (x, y, z)]
    if pt is None:
        x, y, z = z, (z[1], z[0]), (0, 0)
    else:
        z2 = pr.f2_mul(z, z)
        x, y = pr.f2_mul(pt[0], z2), pr.f2_mul(pt[1], pr.f2_mul(z2, z))
    return [pr.fq_to_mont(c) for v in (x, y, z) for c in v]


def _affine(group, w):
    """plain affine point of flat Montgomery Jacobian coordinates; None: Z = 0"""
    v = [pr.fq_from_mont(c) for c in w]
    if group == "g1":
        x, y, z = v
        if z == 0:
            return None
        zi = pow(z, -1, P)
        return (x * zi * zi % P, y * zi * zi * zi % P)
    x, y, z = (v[0], v[1]), (v[2], v[3]), (v[4], v[5])
    if z == (0, 0):
        return None
    zi = pr.f2_inv(z)
    zi2 = pr.f2_mul(zi, zi)
    return (pr.f2_mul(x, zi2), pr.f2_mul(y, pr.f2_mul(zi2, zi)))


def _wave_cases(group):
    g = random.Random(0x3A7E if group == "g1" else 0x3A7F)
    mul, add, neg, gen = (pr.g1_mul, pr.g1_add, pr.g1_neg, pr.G1) if group == "g1" else (pr.g2_mul, pr.g2_add, pr.g2_neg, pr.G2)
    rz = (lambda: g.randrange(1, P)) if group == "g1" else (lambda: (g.randrange(P), g.randrange(1, P)))
    one = 1 if group == "g1" else (1, 0)
    pts = [mul(k, gen) for k in (1, 2, 3, 0xdeadbeef, 2 ** 200 + 7, pr.R - 1)]
    dbl, adds = [], []
    for i, a in enumerate(pts):
        dbl.append((a, rz() if i else one, add(a, a), "dbl"))
        for j, b in enumerate(pts):
            if i != j and add(a, b) is not None:
                adds.append((a, rz(), b, rz() if (i + j) % 3 else one, add(a, b), "generic"))
        adds.append((a, rz(), a, rz(), add(a, a), "P + P: the doubling branch"))
        adds.append((a, rz(), neg(a), rz(), None, "P + (-P)"))
    a = pts[3]
    dbl.append((None, rz(), None, "dbl(inf)"))
    adds += [(None, rz(), a, rz(), a, "inf + P"), (a, rz(), None, rz(), a, "P + inf"), (None, rz(), None, rz(), None, "inf + inf"),
             (pts[0], one, pts[5], one, None, "G + (r-1) G, Z = 1")]
    return dbl, adds


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["g1", "g2"])
def test_wave_formulas(run, group):
    """wave::jdbl / jadd: all four rows hold the same words, the words equal the scalar jac_dbl /
    jac_add of the same input (the header's claim), the affine value is pyref's group law and
    infinity is Z = 0"""
    dbl, adds = _wave_cases(group)
    nw = 36 if group == "g1" else 72
    op = WAVE + (0 if group == "g1" else 2)
    for kind, cases, rows in (("jdbl", dbl, [_jac(group, a, z) for a, z, _, _ in dbl]),
                              ("jadd", adds, [_jac(group, a, za) + _jac(group, b, zb) for a, za, b, zb, _, _ in adds])):
        o = run(op + (kind == "jadd"), rows)
        for i, c in enumerate(cases):
            blocks = [o[i, nw * k:nw * (k + 1)] for k in range(5)]
            for k in (1, 2, 3):
                assert np.array_equal(blocks[k], blocks[0]), (kind, c[-1], "row", k)
            assert np.array_equal(blocks[4], blocks[0]), (kind, c[-1], "wave vs scalar")
            coords = [fc.val(blocks[0][12 * s:12 * s + 12].astype(object)) for s in range(nw // 12)]
            assert all(v < P for v in coords), (kind, c[-1], "canonical")
            assert _affine(group, coords) == c[-2], (kind, c[-1])
