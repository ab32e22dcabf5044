// mbls_sqrt.hpp -- square roots in Fq and in the pair-sliced Fq2 (p == 3 mod 4), for the point
// decompression of serde.hip.  (No reference counterpart: the reference has no square root.)
//
// One exponentiation serves both: t = a^((p - 3) / 4).  For a != 0, s = t a = a^((p + 1) / 4) is a
// root of a exactly when a is a square, and then t s = a^((p - 1) / 2) = 1: t is also 1 / s, which
// is the division the Fq2 root needs, so no inversion runs anywhere.
//
// The chain.  The exponent is a constant, the same bits in every lane: the chain is a sliding
// window over it, recoded AT COMPILE TIME into a schedule of (squarings, odd multiplier) steps that
// the kernel walks with wave-uniform scalar reads -- no lane ever takes a branch another lane of
// its wave does not.  The table of odd powers a, a^3, .. a^(2^W - 1) lives in registers: each
// entry has a name the compiler sees (an unrolled chain of wave-uniform tests picks the product's
// site), never an index computed at run time, which would send the table to scratch.  The chain
// runs on the radix-2^28 products of mbls_fq28.hpp inside their documented invariants: the input
// comes through unpack_shift8 (normalised, < 256 p), every later operand is a product's output
// (normalised, < 27 p after the first level, < 2 p from then on), and the result leaves through
// to_words as canonical Montgomery words.  Everything around the chain -- the radicand, the root's
// check s^2 == a, the choice of sign -- uses the generic Fq / PFq2 operators, whose results are
// canonical, so every equality is taken on canonical words.
//
// Window width (MBLS_SQRT_WINDOW, measured in DESIGN.md 5.8), squarings + products with the table's
// own: 1 is plain binary square-and-multiply (378 + 227 = 605), 2 the odd table {a, a^3} (521),
// 3 {a, a^3, a^5, a^7} (377 + 105 + 4 = 486), 4 eight entries, 112 registers of table (375 + 78 + 8
// = 461).  The time follows the count, not the occupancy (5 waves per SIMD at width 1, 2 at width
// 4), so 4 is the default; no width has scratch.
#pragma once
#include "mbls_fq28.hpp"
#include "mbls_pairfield.hpp"

#ifndef MBLS_SQRT_WINDOW
#define MBLS_SQRT_WINDOW 4
#endif

namespace mbls {
namespace fsqrt {

constexpr int EXP_BITS = 379;  // (p - 3) / 4 < 2^379
// bit i of (p - 3) / 4 = bit i + 2 of p - 3; p ends in ..aaab, so p - 3 only changes the low word
constexpr uint32_t exp_bit(int i) {
    const int b = i + 2, w = b >> 5;
    const uint32_t word = w == 0 ? FqCfg::MOD[0] - 3u : (w < 12 ? FqCfg::MOD[w] : 0u);
    return (word >> (b & 31)) & 1u;
}

// One step: `nsq` squarings, then a product with table entry `idx` (a^(2 idx + 1)); NONE: no product
// (the exponent's trailing zeros).  The first step only loads its entry.
constexpr uint32_t NONE = 0xff;
template <int W>
struct Schedule {
    uint16_t op[EXP_BITS + 1];  // nsq | idx << 8
    int n;
};
template <int W>
constexpr Schedule<W> make_schedule() {
    Schedule<W> s{};
    int n = 0, i = EXP_BITS - 1, nsq = 0;
    while (i >= 0 && !exp_bit(i)) --i;
    while (i >= 0) {
        if (!exp_bit(i)) {
            ++nsq;
            --i;
            continue;
        }
        int lo = i - W + 1 < 0 ? 0 : i - W + 1;  // the longest window [lo, i] that ends in a set bit
        while (!exp_bit(lo)) ++lo;
        uint32_t v = 0;
        for (int k = i; k >= lo; --k) v = (v << 1) | exp_bit(k);
        nsq += i - lo + 1;
        s.op[n] = (uint16_t)((n == 0 ? 0 : nsq) | ((v >> 1) << 8));
        ++n;
        nsq = 0;
        i = lo - 1;
    }
    if (nsq) s.op[n++] = (uint16_t)(nsq | (NONE << 8));
    s.n = n;
    return s;
}
template <int W>
__device__ constexpr Schedule<W> SCHEDULE = make_schedule<W>();

// a^((p - 3) / 4) for canonical Montgomery words a (any value, 0 -> 0), canonical Montgomery words
template <int W = MBLS_SQRT_WINDOW>
MBLS_DEV Fq pow_p34(const Fq& a) {
    using namespace r28;
    constexpr int T = 1 << (W - 1);
    F28 tbl[T];
    tbl[0] = unpack_shift8(a.v);
    if constexpr (T > 1) {
        const F28 a2 = sqr(tbl[0]);
#pragma unroll
        for (int k = 1; k < T; ++k) tbl[k] = mul(tbl[k - 1], a2);
    }
    const Schedule<W>& S = SCHEDULE<W>;
    F28 acc = tbl[0];
    {
        const uint32_t first = S.op[0] >> 8;
#pragma unroll
        for (int k = 1; k < T; ++k)
            if (first == (uint32_t)k) acc = tbl[k];
    }
#pragma unroll 1
    for (int j = 1; j < S.n; ++j) {
        const uint32_t op = S.op[j], idx = op >> 8;
#pragma unroll 1
        for (uint32_t q = op & 0xff; q; --q) acc = sqr(acc);
#pragma unroll
        for (int k = 0; k < T; ++k)
            if (idx == (uint32_t)k) acc = mul(acc, tbl[k]);
    }
    Fq r;
    to_words(acc, r.v);
    return r;
}

// s = a^((p + 1) / 4) and t = a^((p - 3) / 4); true when s^2 == a, i.e. a is a square (0 included:
// s = t = 0); then t = 1 / s for a != 0
MBLS_DEV bool root(Fq& s, Fq& t, const Fq& a) {
    t = pow_p34(a);
    s = t * a;
    return sqr(s) == a;
}

// a / 2 on canonical words of either form: (a + p) / 2 for an odd a
MBLS_DEV Fq half(const Fq& a) {
    const uint32_t mask = 0u - (a.v[0] & 1u);
    Fq r;
    unsigned carry = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) r.v[i] = __builtin_addc(a.v[i], FqCfg::MOD[i] & mask, carry, &carry);
    // a + p < 2^382: no carry out of the top word
#pragma unroll
    for (int i = 0; i < 11; ++i) r.v[i] = __builtin_amdgcn_alignbit(r.v[i + 1], r.v[i], 1);
    r.v[11] >>= 1;
    return r;
}

// is the canonical STANDARD-form y the larger of {y, p - y}: y > (p - 1) / 2, i.e. 2 y >= p
MBLS_DEV bool is_larger_half(const Fq& y) {
    const Fq d = x2_in(y);  // < 2^382
    uint32_t t[12];
    return sub_mod_raw<FqCfg>(t, d.v) == 0;
}

MBLS_DEV bool pair_any(bool p) {
    const uint32_t v = p ? 1u : 0u;
    return (v | pairdpp::swap(v)) != 0;
}
MBLS_DEV bool pair_all(bool p) {
    const uint32_t v = p ? 1u : 0u;
    return (v & pairdpp::swap(v)) != 0;
}
// the value of `p` on the pair's odd (c1) / even (c0) lane, on both lanes.  The swap runs first, on
// both lanes: inside a `?:` arm only one lane of the pair would execute it, and a DPP move reads
// nothing from a lane that is switched off.
MBLS_DEV uint32_t pair_odd(uint32_t v) {
    const uint32_t w = pairdpp::swap(v);
    return pairdpp::odd() ? v : w;
}
MBLS_DEV uint32_t pair_even(uint32_t v) {
    const uint32_t w = pairdpp::swap(v);
    return pairdpp::odd() ? w : v;
}
MBLS_DEV bool pair_odd(bool p) { return pair_odd(p ? 1u : 0u) != 0; }
MBLS_DEV bool pair_even(bool p) { return pair_even(p ? 1u : 0u) != 0; }

// Root of the pair-sliced a = a0 + a1 u (canonical Montgomery), by the norm: with n^2 = a0^2 + a1^2
// and a1 != 0 exactly one of d+ = (a0 + n) / 2, d- = (a0 - n) / 2 is a square (their product is
// -a1^2 / 4 and -1 is not a square), and for that d = x0^2 the root is x0 + a1 / (2 x0) u.  The
// even lane tries d+ and the odd lane d- in the SAME exponentiation; the lane whose candidate is
// a square holds x0 and 1 / x0 (root() above), finishes both components and hands the partner
// its one.  a1 == 0 (the radicand is real): the lanes try a0 and -a0 instead, of which exactly one
// is a square for a0 != 0, and the root is (x0, 0) or (0, x0); the norm's root is not needed.
// Returns false when a is not a square (the norm is not one).  Every predicate that steers
// control flow is combined over the pair.
MBLS_DEV bool root(PFq2& y, const PFq2& a) {
    const bool odd = pairdpp::odd();
    const Fq other = partner(a.v);
    const Fq a0 = select(odd, other, a.v), a1 = select(odd, a.v, other);
    const bool real = pair_odd(a.v.is_zero());  // a1 == 0
    Fq d;
    if (real) {
        d = select(odd, neg(a0), a0);
    } else {
        Fq n, t;
        if (!root(n, t, sqr(a0) + sqr(a1))) return false;  // the same value on both lanes
        d = half(select(odd, a0 - n, a0 + n));
    }
    Fq x0, t;
    const bool win = root(x0, t, d);
    // this lane's finished root (k0, k1), valid where `win`
    const Fq k1 = real ? Fq::zero() : half(a1 * t);
    const Fq keep = select(odd, k1, x0), give = partner(select(odd, x0, k1));
    if (real) {
        // (x0, 0) from the even lane or (0, x0) from the odd one; a0 == 0: both are zero
        y.v = win ? x0 : Fq::zero();
        return pair_any(win);
    }
    y.v = select(win, keep, give);
    return pair_any(win);
}

}  // namespace fsqrt
}  // namespace mbls
