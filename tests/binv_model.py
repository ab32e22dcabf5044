"""csrc/mbls_binv.hpp `binv::inverse<N>` restated on plain Python integers, with a trace of the
events inside it and with mutants of its sign correction.

The approximate binary GCD runs K = 30 inner steps on 64-bit approximations of (a, b) (the low 31
bits, the top 33 bits of max(bitlen(a | b), 64) bits).  The approximation can order a and b the
wrong way; f a + g b then comes out negative, the magnitude is kept and the row (f, g) is negated
before it is applied to (u, v), one outer step late (the software-pipelined pending update).  Those
negations are the routine's only data-dependent branches.

`inverse(y, m)` returns (1 / y mod m, outer steps, trace).  trace[k] describes outer step k + 1:
    neg_a, neg_b   lincomb_shift returned true for a' (row f0, g0) / b' (row f1, g1)
    clamped        bitlen(a | b) < 64: n was clamped to 64
    xeq            the approximations entered the inner loop equal
    updates        [(negative sum, final subtractions)] of the two (u, v) updates issued in this step
and trace[-1] is {"final": (negative sum, final subtractions)} of the last update of v.

`mutant=` breaks the sign correction the way a wrong kernel could (no mutated kernel is built):
    drop_a          a's correction is ignored
    drop_b          b's correction is ignored
    early           the negation goes to the row applied in the same step, not to the pending one
    lane0_for_both  the four-lane form reading lane 0's flag for both rows"""
K = 30
MUTANTS = ("drop_a", "drop_b", "early", "lane0_for_both")


def corrections(trace):
    """[(row, outer step)] of a trace, in the order the harness's trace mode prints them"""
    out = []
    for k, t in enumerate(trace[:-1]):
        out += [(row, k + 1) for row in "ab" if t["neg_" + row]]
    return out


def _approx(x, n):
    return (x & 0x7fffffff) | (((x >> (n - 33)) & ((1 << 33) - 1)) << 31)


def _lincomb_shift(a, b, f, g):
    s = f * a + g * b
    assert s % (1 << K) == 0
    return abs(s) >> K, s < 0  # a zero sum is never negative here


def _lincomb_mod(u, v, f, g, m, ninv):
    s = f * u + g * v
    neg = s < 0
    if neg:
        s += m << (K + 1)
        assert s >= 0
    k = ((s & 0xffffffff) * ninv) & ((1 << K) - 1)
    t = s + k * m
    assert t % (1 << K) == 0
    t >>= K
    subs = 0
    for _ in range(2):
        if t >= m:
            t -= m
            subs += 1
    assert t < m
    return t, (neg, subs)


def inverse(y, m, mutant=None):
    assert mutant is None or mutant in MUTANTS
    assert 0 < y < m and m & 1
    N = (m.bit_length() + 31) // 32
    ninv = -pow(m, -1, 1 << 32) % (1 << 32)
    a, b, u, v = y, m, 1, 0
    pf0, pg0, pf1, pg1 = 1 << K, 0, 0, 1 << K  # the pending (u, v) update
    steps, cap, trace = 0, (64 * N) // K + 8, []
    while a and steps < cap:
        steps += 1
        nl = (a | b).bit_length()
        n = max(nl, 64)
        xa, xb = _approx(a, n), _approx(b, n)
        ev = {"clamped": nl < 64, "xeq": xa == xb}
        f0, g0, f1, g1 = 1, 0, 0, 1
        for _ in range(K):
            odd, lt = xa & 1, xa < xb
            if odd and lt:
                f0, g0, f1, g1 = f1, g1, f0, g0
                xa, xb = xb, xa  # now xa - xb = the former xb - xa
            if odd:
                xa -= xb
                f0, g0 = f0 - f1, g0 - g1
            xa >>= 1
            f1, g1 = 2 * f1, 2 * g1
        assert max(abs(f0), abs(g0), abs(f1), abs(g1)) <= 1 << K
        na, neg_a = _lincomb_shift(a, b, f0, g0)
        nb, neg_b = _lincomb_shift(a, b, f1, g1)
        ev["neg_a"], ev["neg_b"] = neg_a, neg_b
        fix_a = neg_a and mutant != "drop_a"
        fix_b = (neg_a if mutant == "lane0_for_both" else neg_b) and mutant != "drop_b"
        if mutant == "early":  # the row applied in this step takes the negation
            if fix_a:
                pf0, pg0 = -pf0, -pg0
            if fix_b:
                pf1, pg1 = -pf1, -pg1
            fix_a = fix_b = False
        nu, e0 = _lincomb_mod(u, v, pf0, pg0, m, ninv)
        nv, e1 = _lincomb_mod(u, v, pf1, pg1, m, ninv)
        ev["updates"] = [e0, e1]
        if fix_a:
            f0, g0 = -f0, -g0
        if fix_b:
            f1, g1 = -f1, -g1
        a, b, u, v = na, nb, nu, nv
        pf0, pg0, pf1, pg1 = f0, g0, f1, g1
        trace.append(ev)
    out, e = _lincomb_mod(u, v, pf1, pg1, m, ninv)
    trace.append({"final": e})
    return out, steps, trace
