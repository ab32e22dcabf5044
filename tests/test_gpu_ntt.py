"""The NTT's lazy butterflies at their reduction boundaries, and the option combinations the prover uses.

k_ntt_pass (csrc/ntt.hip) keeps values in [0, 2r) between the first load and the last store.  Its
exact-boundary cases -- a + b == 2r in add_2r, a == b in sub_2r, a value that reaches the last
store as exactly r (reduce_once forward, the reducing product by n^-1 inverse) -- are never
reached by uniformly random data, so a kernel that decides any of them the wrong way passes every
random-input parity test.  Structured inputs reach them by the hundred.  tests/ntt_model.py
restates the pass in Python integers and counts the events (forward transform, seed-7 random):

    input, size                 add_eq_2r   sub_eq   store_eq_r   add_carry
    random, 2^9                         0        0            0         352
    random, 2^12                        0        0            0        4000
    freq_5 (w^(5i)), 2^9              389     1393          230           9
    freq_5, 2^12                     4563    16129          108          97
    const_r-1, 2^9                     57     2189            1         145
    const_r-1, 2^12                   460    23655            1        1160
    alternating +1 -1, 2^9             38     2227            1          89
    alternating, 2^12                 307    23961            2         716

(inverse: freq_5 338 / 1449 / 214 at 2^9 and 3651 / 16011 / 1517 at 2^12; the constant and
alternating inputs are their own mirror images and count the same both ways.)

The model's mutants (one boundary decided the wrong way each; no mutated kernel is ever built):
reduce_once with > for >=, add_2r keeping a sum of 2r, sub_2r adding 2r when a == b.  Observed at
2^9 and 2^12: random inputs catch none of the three, forward or inverse; the constant,
alternating, one- and two-frequency inputs catch all three forward (the inverse's reducing
product hides the add / sub mutants, and shows the reduce_once one).  The fourth mutant, add_2r
ignoring the carry out of 2^256, is caught by random data.

CPU tests: ntt.hip's constants, the model against pyref and against the closed forms, the
coverage condition above, the negative control.  GPU tests (-m gpu): every structured family
through the real kernel at one size per pass-plan shape, the coset x ordering x columns_batch x
direction x placement product, the pass plans no other test runs against the oracle, and the zero
coset generator."""
import functools
import itertools
import re

import numpy as np
import pytest

import helpers as H
import ntt_model as M
from helpers import pyref as pr

R = pr.R
gpu = pytest.mark.gpu
MODEL_SIZES = [1, 2, 3, 8, 9, 12]
STRUCTURED_SIZES = M.ORACLE_CHECKED_LOG_N["test_gpu_ntt::test_structured_families_device"]


def _random_mont(seed, n):
    g = pr.rng(seed)
    return [pr.fr_to_mont(g.randrange(R)) for _ in range(n)]


# ----------------------------------------------------------------------------- constants (CPU)
def _words(src, name):
    m = re.search(r"\b" + name + r"\[[^\]]*\]\s*=\s*\{([^}]*)\}", src)
    assert m, name
    return [int(v.strip().rstrip("uUlL"), 16) for v in m.group(1).split(",") if v.strip()]


def test_ntt_constants():
    src = open(M.NTT_HIP).read()
    val = lambda name, bits: sum(v << (bits * i) for i, v in enumerate(_words(src, name)))
    assert val("NTT_TWO_R", 32) == 2 * R and len(_words(src, "NTT_TWO_R")) == 8
    assert val("HFR_P", 64) == R
    assert val("HFR_ONE", 64) == (1 << 256) % R
    assert val("HFR_R2", 64) == (1 << 512) % R
    assert val("ROOT_2_32_MONT", 64) == pr.fr_to_mont(pr.ROOT_OF_UNITY)
    assert pow(pr.ROOT_OF_UNITY, 1 << 31, R) == R - 1  # primitive 2^32-th root
    assert M.kernel_defaults() == (10, 8)  # the header comment and the plans below speak of these


def test_pass_plans_of_the_gpu_sizes():
    """each structured size is there for a shape of the plan: (s0, L, logC) per pass"""
    assert M.plan(1) == [(0, 1, 0)]   # lone radix-2 stage, multiply skipped
    assert M.plan(2) == [(0, 2, 0)]   # the trivial pair only
    assert M.plan(3) == [(0, 3, 0)]   # trivial pair + radix-2 tail
    assert M.plan(8) == [(0, 8, 0)]   # the largest single pass
    assert M.plan(9) == [(0, 5, 4), (5, 4, 5)]    # partial tiles (2^9 < 2^10), logC clamped
    assert M.plan(12) == [(0, 6, 4), (6, 6, 4)]   # full tiles
    assert M.plan(13) == [(0, 7, 3), (7, 6, 4)]   # odd L in a first pass that is not the last
    assert M.plan(17) == [(0, 6, 4), (6, 6, 4), (12, 5, 5)]  # first plan with a middle pass
    for k in range(1, 31):
        p = M.plan(k)
        assert sum(L for _, L, _ in p) == k and all(1 <= L <= 8 and 0 <= c and L + c <= 10 for _, L, c in p)


def test_oracle_checked_sizes_cover_every_log_n():
    sizes = set(itertools.chain.from_iterable(M.ORACLE_CHECKED_LOG_N.values()))
    assert sizes >= set(range(25)), sorted(set(range(25)) - sizes)


# ----------------------------------------------------------------------------- the model (CPU)
@pytest.mark.parametrize("log_n", MODEL_SIZES)
def test_model_matches_reference_and_closed_forms(log_n):
    n = 1 << log_n
    x = _random_mont(7 + log_n, n)
    xs = [pr.fr_from_mont(v) for v in x]
    for inverse, ref in ((False, pr.ntt_forward), (True, pr.ntt_inverse)):
        out, _ = M.run(x, inverse)
        assert [pr.fr_from_mont(v) for v in out] == ref(xs), inverse
    names = set()
    for f in M.families(log_n):
        names.add(f.name)
        fs = [pr.fr_from_mont(v) for v in f.x]
        for inverse, ref in ((False, pr.ntt_forward), (True, pr.ntt_inverse)):
            want = f.expect(inverse)
            assert all(0 <= v < R for v in want)
            assert [pr.fr_from_mont(v) for v in want] == ref(fs), (f.name, inverse)  # the closed form itself
            out, _ = M.run(f.x, inverse)
            assert out == want, (f.name, inverse)
    assert len(names) == len(M.families(log_n)) and {"zeros", "const_r-1", "alternating", "two_freq"} <= names


@pytest.mark.parametrize("log_n", [9, 12])
def test_structured_inputs_reach_the_boundaries(log_n):
    """the coverage condition: the inputs the GPU tests feed reach every boundary in the model.
    Observed (forward; add_eq_2r / sub_eq / store_eq_r): freq_5 389 / 1393 / 230 at 2^9 and
    4563 / 16129 / 108 at 2^12; const_r-1 57 / 2189 / 1 and 460 / 23655 / 1; alternating
    38 / 2227 / 1 and 307 / 23961 / 2; random 0 / 0 / 0 at both."""
    for inverse in (False, True):
        _, ev = M.run(M.family(log_n, "freq_5").x, inverse)
        assert ev["add_eq_2r"] > 0 and ev["sub_eq"] > 0 and ev["store_eq_r"] > 0, (inverse, ev)
        assert ev["mul_in_ge_r"] > 0 and ev["store_ge_r"] >= ev["store_eq_r"]
    for name in ("const_1", "const_r-1", "const_rand", "alternating"):
        _, ev = M.run(M.family(log_n, name).x, False)
        assert ev["add_eq_2r"] > 0 and ev["sub_eq"] > 0, (name, ev)
    # the families together also carry out of 2^256 in add_2r (random data does that by itself)
    assert M.run(M.family(log_n, "two_freq").x, False)[1]["add_carry"] > 0


def test_boundary_mutants_are_caught():
    """negative control at 2^9: each boundary mutant gives a wrong output for at least one
    structured family (forward), the carry mutant for random data.  Observed, not asserted:
    random data catches none of the three boundary mutants."""
    fams = [f for f in M.families(9) if f.name.split("_")[0] in ("const", "alternating", "freq", "two")]
    for mutant in ("reduce_gt", "add_keep_2r", "sub_eq_adds"):
        caught = [f.name for f in fams if M.run(f.x, False, mutant=mutant)[0] != f.fwd]
        assert caught, mutant
        assert "freq_5" in caught, (mutant, caught)  # the one input the coverage condition pins
    # the inverse's last store: r n^-1 leaves fips::mul's accumulator at exactly r
    f = M.family(9, "freq_5")
    assert M.run(f.x, True, mutant="reduce_gt")[0] != f.inv
    x = _random_mont(7, 512)
    for inverse in (False, True):
        assert M.run(x, inverse, mutant="add_no_carry")[0] != M.run(x, inverse)[0], inverse


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gpu_helpers
    gpu_helpers.amd.lib()
    gpu_helpers.amd.ntt_init_domain()
    return gpu_helpers.amd


def _oracle_threads(log_n):
    return 16 if log_n >= 16 else 1


def _family_arrays(log_n):
    return [(f.name, M.to_limbs(f.x), M.to_limbs(f.fwd), M.to_limbs(f.inv)) for f in M.families(log_n)]


_small_family_arrays = functools.lru_cache(maxsize=None)(_family_arrays)


def _device_both_ways(amd, x, inverse, batch=1):
    """x (host) through the device transform out of place and in place -> two host arrays"""
    import torch
    d = amd.torch_u64(x)
    y = torch.zeros_like(d)
    amd.ntt(d, inverse=inverse, out=y, batch=batch)
    z = d.clone()
    amd.ntt(z, inverse=inverse, out=z, batch=batch)
    torch.cuda.synchronize()
    assert np.array_equal(amd.to_numpy_u64(d), x), "out-of-place transform wrote its input"
    return amd.to_numpy_u64(y), amd.to_numpy_u64(z)


@gpu
@pytest.mark.parametrize("log_n", STRUCTURED_SIZES)
def test_structured_families_device(amd, log_n):
    """every family, forward and inverse, out of place and in place: kernel == closed form ==
    oracle, bit for bit (the closed form is canonical by construction)"""
    fams = _small_family_arrays(log_n) if log_n <= 13 else _family_arrays(log_n)
    for name, x, fwd, inv in fams:
        for inverse, want in ((False, fwd), (True, inv)):
            assert np.array_equal(H.oracle_ntt(x, log_n, inverse, threads=_oracle_threads(log_n)), want), \
                (name, inverse, "oracle vs closed form")
            oop, inp = _device_both_ways(amd, x, inverse)
            assert np.array_equal(oop, want), (name, inverse, "out of place")
            assert np.array_equal(inp, want), (name, inverse, "in place")


@gpu
@pytest.mark.parametrize("log_n", [9, 12, 13])
def test_structured_batch_of_three_families(amd, log_n):
    """one launch, three different families: a wrong polynomial offset leaks across members"""
    fams = {f[0]: f for f in _small_family_arrays(log_n)}
    pick = [fams[k] for k in ("const_r-1", "freq_5", "delta_1_r-1")]
    x = np.ascontiguousarray(np.concatenate([f[1] for f in pick]))
    for inverse in (False, True):
        want = np.concatenate([f[3 if inverse else 2] for f in pick])
        oop, inp = _device_both_ways(amd, x, inverse, batch=3)
        assert np.array_equal(oop, want), inverse
        assert np.array_equal(inp, want), inverse


# ---- the option cross-product -------------------------------------------------------------
ORDERINGS = ["NN", "NR", "RN", "RR", "NM", "MN"]
GENS = {"absent": None, "one": pr.FR_R, "seven": pr.fr_to_mont(7), "root_2_10": pr.fr_to_mont(pr.omega(10))}
BATCH = 3


def _gen_limbs(name):
    g = GENS[name]
    return None if g is None else np.array(pr.int_to_limbs(g, 4), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _polys(log_n):
    """BATCH random polynomials, canonical Montgomery, as lists of ints"""
    return tuple(tuple(_random_mont(0xC05E7 + 16 * log_n + b, 1 << log_n)) for b in range(BATCH))


@functools.lru_cache(maxsize=None)
def _coset_expected(log_n, gen, inverse):
    """natural-order transforms of _polys from the oracle and Python scaling alone: forward
    NTT(x_i g^i), inverse g^-i INTT(X)_i (Montgomery data times a standard-form power)"""
    n = 1 << log_n
    g = 1 if GENS[gen] is None else pr.fr_from_mont(GENS[gen])
    pw = M._powers(pow(g, -1, R) if inverse else g, n)
    out = []
    for p in _polys(log_n):
        if inverse:
            y = M.from_limbs(H.oracle_ntt(M.to_limbs(p), log_n, True, threads=1))
            out.append(M.to_limbs([(v * t) % R for v, t in zip(y, pw)]))
        else:
            out.append(H.oracle_ntt(M.to_limbs([(v * t) % R for v, t in zip(p, pw)]), log_n, False, threads=1))
    return tuple(out)


def _layout(members, log_n, rev, cols):
    """members (natural order, (n, 4) each) -> the call's buffer: bit-reversed element order,
    row-major batch or columns_batch (element i of member b at i * batch + b)"""
    perm = M.bitrev_perm(log_n)
    ms = [m[perm] if rev else m for m in members]
    if cols:
        return np.ascontiguousarray(np.stack(ms, axis=1).reshape(len(ms) << log_n, 4))
    return np.ascontiguousarray(np.concatenate(ms))


def _call(amd, buf, placement, **kw):
    import torch
    if placement == "host":
        return amd.ntt(buf.copy(), **kw)
    d = amd.torch_u64(buf)
    out = d if placement == "inplace" else torch.zeros_like(d)
    amd.ntt(d, out=out, **kw)
    torch.cuda.synchronize()
    if placement != "inplace":
        assert np.array_equal(amd.to_numpy_u64(d), buf), "input overwritten"
    return amd.to_numpy_u64(out)


def _case(log_n, gen, ordering, cols, inverse):
    """(input buffer, expected output buffer, keywords) of one option combination"""
    x = [M.to_limbs(p) for p in _polys(log_n)]
    buf = _layout(x, log_n, ordering[0] in "RM", cols)
    want = _layout(_coset_expected(log_n, gen, inverse), log_n, ordering[1] in "RM", cols)
    kw = dict(inverse=inverse, batch=BATCH, ordering=ordering, columns_batch=cols)
    if GENS[gen] is not None:
        kw["coset_gen"] = _gen_limbs(gen)
    return buf, want, kw


@gpu
@pytest.mark.parametrize("ordering", ORDERINGS)
@pytest.mark.parametrize("gen", list(GENS))
def test_option_product(amd, gen, ordering):
    """coset generator x ordering x columns_batch x direction x placement at 2^9, batch 3"""
    for cols, inverse, placement in itertools.product((False, True), (False, True), ("host", "device", "inplace")):
        buf, want, kw = _case(9, gen, ordering, cols, inverse)
        assert np.array_equal(_call(amd, buf, placement, **kw), want), (cols, inverse, placement)


def test_option_product_expected_is_not_vacuous():
    """the expectations differ where the options differ (an expected value that ignored the
    generator or the ordering would let a kernel that ignores them pass)"""
    a = _case(9, "absent", "NN", False, False)[1]
    assert np.array_equal(a, _case(9, "one", "NN", False, False)[1])
    for other in (("seven", "NN", False), ("root_2_10", "NN", False), ("absent", "NR", False), ("absent", "NN", True)):
        assert not np.array_equal(a, _case(9, *other, False)[1]), other
    assert not np.array_equal(_case(9, "seven", "NN", False, True)[1], _case(9, "absent", "NN", False, True)[1])


@gpu
@pytest.mark.parametrize("cols", [False, True])
@pytest.mark.parametrize("gen", ["one", "seven", "root_2_10"])
def test_coset_one_is_plain_and_round_trips(amd, gen, cols):
    for ordering, back in (("NN", "NN"), ("NR", "RN"), ("RR", "RR")):
        buf, _, kw = _case(9, gen, ordering, cols, False)
        fwd = _call(amd, buf, "device", **kw)
        if gen == "one":
            plain = dict(kw)
            del plain["coset_gen"]
            assert np.array_equal(fwd, _call(amd, buf, "device", **plain)), ordering
        kw.update(inverse=True, ordering=back)
        for placement in ("device", "inplace"):
            assert np.array_equal(_call(amd, fwd, placement, **kw), buf), (ordering, placement)


@gpu
@pytest.mark.parametrize("entry", ["coset", "field"])
def test_other_entry_points_give_the_same_bytes(amd, entry):
    """bls12_381_coset_ntt_cuda (generator as an argument) and bls12_381_field_ntt_cuda against
    bls12_381_ntt_cuda and the expectation"""
    for gen, ordering, cols, inverse in itertools.product(("absent", "seven", "root_2_10"), ("NN", "RR"),
                                                          (False, True), (False, True)):
        buf, want, kw = _case(9, gen, ordering, cols, inverse)
        for placement in ("host", "inplace"):
            got = _call(amd, buf, placement, entry=entry, **kw)
            assert np.array_equal(got, _call(amd, buf, placement, entry="ntt", **kw)), (gen, ordering, cols, inverse)
            assert np.array_equal(got, want), (gen, ordering, cols, inverse, placement)


@gpu
def test_coset_rr_columns_inplace_2_12(amd):
    for gen in ("seven", "root_2_10"):
        for inverse in (False, True):
            buf, want, kw = _case(12, gen, "RR", True, inverse)
            assert np.array_equal(_call(amd, buf, "inplace", **kw), want), (gen, inverse)


@gpu
@pytest.mark.parametrize("entry", ["ntt", "field", "coset"])
def test_zero_coset_generator_is_rejected(amd, entry):
    """a generator that is zero mod r (a zero-initialised NTTConfig) has no inverse"""
    x = M.to_limbs(_random_mont(3, 64))
    for g in (0, R):
        for inverse in (False, True):
            out = np.full_like(x, 0xA5)
            with pytest.raises(amd.IcicleError) as e:
                amd.ntt(x, inverse=inverse, out=out, entry=entry,
                        coset_gen=np.array(pr.int_to_limbs(g, 4), dtype=np.uint64))
            assert e.value.code == amd.INVALID_ARGUMENT, (g, inverse)
            assert np.all(out == 0xA5), "a rejected call wrote its output"
    # the library still works after the rejections
    assert np.array_equal(amd.ntt(x, entry=entry), H.oracle_ntt(x, 6, False, threads=1))


# ---- the pass plans no other test runs against the oracle ---------------------------------
@gpu
@pytest.mark.parametrize("log_n", M.ORACLE_CHECKED_LOG_N["test_gpu_ntt::test_remaining_pass_plans_vs_oracle"])
def test_remaining_pass_plans_vs_oracle(amd, log_n):
    """random data forward against the oracle, exact round trip (as test_gpu_parity's
    test_ntt_vs_oracle): each log_n has its own (s0, L, logC) and so its own index arithmetic"""
    import torch
    n = 1 << log_n
    x = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    amd.gen_scalars(x, 0x5EED0700 + log_n, montgomery=True)
    y = torch.zeros_like(x)
    amd.ntt(x, inverse=False, out=y)
    z = torch.zeros_like(x)
    amd.ntt(y, inverse=True, out=z)
    torch.cuda.synchronize()
    xn = amd.to_numpy_u64(x)
    assert np.array_equal(amd.to_numpy_u64(y), H.oracle_ntt(xn, log_n, False, threads=_oracle_threads(log_n)))
    assert np.array_equal(amd.to_numpy_u64(z), xn)
