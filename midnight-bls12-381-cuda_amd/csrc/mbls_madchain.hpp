// mbls_madchain.hpp -- one column of an unsaturated-radix product as ONE v_mad_u64_u32 chain.
//
// The radix-2^28 Fq (mbls_fq28.hpp) and radix-2^29 Fr (mbls_fr29.hpp) products accumulate each
// column in a single 64-bit register.  Written as C++ additions, LLVM reassociates every column
// into its own fresh chain (first product with a zero addend) and merges the previous column's
// carry with an extra 64-bit add at the end: one v_lshl_add_u64 per column (~27 per Fq product,
// ~17 per Fr product, 6-8% of the instructions; tools/isa counts in DESIGN.md).  The mads here are
// inline asm, each accumulating into the operand the previous one wrote: asm statements are opaque
// to the reassociation, so the column stays the chain the formula is.
//
// Statement boundaries cost.  On gfx950 the compiler cannot see what an asm statement holds and
// pads it with one wait state (`s_nop 0`) whenever the next instruction reads a VGPR it wrote; a
// lone wave on a dependent chain pays for each pad (tools/latbench.hip).  So an Fq
// column (`chain`) is emitted in as few statements as its terms allow: up to MAXP mads per statement (two operands
// each, named, so a statement's text does not depend on how many terms of which kind it holds), a
// longer column split into statements of equal length.  A statement may open with the previous
// column's closing step (`tm * tp` added, then the accumulator shifted right by SH): that step
// depends on a value computed in C++ from the previous statement's result, so carrying it over
// saves the boundary it would otherwise be.  The carry-out v_mad_u64_u32 must name on gfx9 goes to
// vcc, which every statement clobbers and never reads.  The compiler schedules and allocates
// around the statements as usual.
#pragma once
#include "mbls_common.hpp"

namespace mbls {
namespace madc {

constexpr int MAXP = 14;  // mads per statement (28 register operands and the accumulator)

#define MBLS_MADC_ST(A, B) "v_mad_u64_u32 %0, vcc, %[" A "], %[" B "], %0\n\t"
// text and operands of term i: V both factors in VGPRs, S the second a wave-uniform constant (SGPR)
#define MBLS_MADC_VT(i) MBLS_MADC_ST("x" #i, "y" #i)
#define MBLS_MADC_SV(i) MBLS_MADC_ST("m" #i, "p" #i)
#define MBLS_MADC_VP(i) , [x##i] "v"(va[i]), [y##i] "v"(vb[i])
#define MBLS_MADC_SP(i) , [m##i] "v"(sa[i]), [p##i] "s"(sb[i])
#define MBLS_MADC_REP0(F)
#define MBLS_MADC_REP1(F) F(0)
#define MBLS_MADC_REP2(F) MBLS_MADC_REP1(F) F(1)
#define MBLS_MADC_REP3(F) MBLS_MADC_REP2(F) F(2)
#define MBLS_MADC_REP4(F) MBLS_MADC_REP3(F) F(3)
#define MBLS_MADC_REP5(F) MBLS_MADC_REP4(F) F(4)
#define MBLS_MADC_REP6(F) MBLS_MADC_REP5(F) F(5)
#define MBLS_MADC_REP7(F) MBLS_MADC_REP6(F) F(6)
#define MBLS_MADC_REP8(F) MBLS_MADC_REP7(F) F(7)
#define MBLS_MADC_REP9(F) MBLS_MADC_REP8(F) F(8)
#define MBLS_MADC_REP10(F) MBLS_MADC_REP9(F) F(9)
#define MBLS_MADC_REP11(F) MBLS_MADC_REP10(F) F(10)
#define MBLS_MADC_REP12(F) MBLS_MADC_REP11(F) F(11)
#define MBLS_MADC_REP13(F) MBLS_MADC_REP12(F) F(12)
#define MBLS_MADC_REP14(F) MBLS_MADC_REP13(F) F(13)

// one statement: [tm * tp, >> SH,] NV terms va[i] vb[i], then NS terms sa[i] sb[i], in that order
#define MBLS_MADC_CASE(V, S)                                                                                       \
    if constexpr (NV == V && NS == S) {                                                                            \
        if constexpr (TAIL)                                                                                        \
            asm(MBLS_MADC_ST("tm", "tp") "v_lshrrev_b64 %0, %[sh], %0\n\t" MBLS_MADC_REP##V(MBLS_MADC_VT)          \
                    MBLS_MADC_REP##S(MBLS_MADC_SV)                                                                 \
                : "+v"(acc)                                                                                        \
                : [sh] "n"(SH), [tm] "v"(tm), [tp] "s"(tp) MBLS_MADC_REP##V(MBLS_MADC_VP) MBLS_MADC_REP##S(MBLS_MADC_SP) \
                : "vcc");                                                                                          \
        else                                                                                                       \
            asm("" MBLS_MADC_REP##V(MBLS_MADC_VT) MBLS_MADC_REP##S(MBLS_MADC_SV)                                   \
                : "+v"(acc)                                                                                        \
                : [sh] "n"(SH) MBLS_MADC_REP##V(MBLS_MADC_VP) MBLS_MADC_REP##S(MBLS_MADC_SP)                       \
                : "vcc");                                                                                          \
    }
// the cases (V, 0) .. (V, n): a statement holds V + S <= MAXP terms, so row V needs S <= MAXP - V only
#define MBLS_MADC_UPTO0(V) MBLS_MADC_CASE(V, 0)
#define MBLS_MADC_UPTO1(V) MBLS_MADC_UPTO0(V) MBLS_MADC_CASE(V, 1)
#define MBLS_MADC_UPTO2(V) MBLS_MADC_UPTO1(V) MBLS_MADC_CASE(V, 2)
#define MBLS_MADC_UPTO3(V) MBLS_MADC_UPTO2(V) MBLS_MADC_CASE(V, 3)
#define MBLS_MADC_UPTO4(V) MBLS_MADC_UPTO3(V) MBLS_MADC_CASE(V, 4)
#define MBLS_MADC_UPTO5(V) MBLS_MADC_UPTO4(V) MBLS_MADC_CASE(V, 5)
#define MBLS_MADC_UPTO6(V) MBLS_MADC_UPTO5(V) MBLS_MADC_CASE(V, 6)
#define MBLS_MADC_UPTO7(V) MBLS_MADC_UPTO6(V) MBLS_MADC_CASE(V, 7)
#define MBLS_MADC_UPTO8(V) MBLS_MADC_UPTO7(V) MBLS_MADC_CASE(V, 8)
#define MBLS_MADC_UPTO9(V) MBLS_MADC_UPTO8(V) MBLS_MADC_CASE(V, 9)
#define MBLS_MADC_UPTO10(V) MBLS_MADC_UPTO9(V) MBLS_MADC_CASE(V, 10)
#define MBLS_MADC_UPTO11(V) MBLS_MADC_UPTO10(V) MBLS_MADC_CASE(V, 11)
#define MBLS_MADC_UPTO12(V) MBLS_MADC_UPTO11(V) MBLS_MADC_CASE(V, 12)
#define MBLS_MADC_UPTO13(V) MBLS_MADC_UPTO12(V) MBLS_MADC_CASE(V, 13)
#define MBLS_MADC_UPTO14(V) MBLS_MADC_UPTO13(V) MBLS_MADC_CASE(V, 14)
template <bool TAIL, int SH, int NV, int NS>
MBLS_DEV void stmt(uint64_t& acc, uint32_t tm, uint32_t tp, const uint32_t* va, const uint32_t* vb, const uint32_t* sa,
                   const uint32_t* sb) {
    static_assert(NV >= 0 && NS >= 0 && (TAIL ? 1 : 0) + NV + NS <= MAXP, "one statement holds at most MAXP mads");
    // the 120 (NV, NS) shapes with NV + NS <= MAXP; the four products of mbls_fq28.hpp use 95 of the
    // 240 statements (tests/test_isa_chains.py restates which: ceil(terms / MAXP) per column, equal lengths)
    MBLS_MADC_UPTO14(0) MBLS_MADC_UPTO13(1) MBLS_MADC_UPTO12(2) MBLS_MADC_UPTO11(3) MBLS_MADC_UPTO10(4)
    MBLS_MADC_UPTO9(5) MBLS_MADC_UPTO8(6) MBLS_MADC_UPTO7(7) MBLS_MADC_UPTO6(8) MBLS_MADC_UPTO5(9)
    MBLS_MADC_UPTO4(10) MBLS_MADC_UPTO3(11) MBLS_MADC_UPTO2(12) MBLS_MADC_UPTO1(13) MBLS_MADC_UPTO0(14)
}
#undef MBLS_MADC_UPTO14
#undef MBLS_MADC_UPTO13
#undef MBLS_MADC_UPTO12
#undef MBLS_MADC_UPTO11
#undef MBLS_MADC_UPTO10
#undef MBLS_MADC_UPTO9
#undef MBLS_MADC_UPTO8
#undef MBLS_MADC_UPTO7
#undef MBLS_MADC_UPTO6
#undef MBLS_MADC_UPTO5
#undef MBLS_MADC_UPTO4
#undef MBLS_MADC_UPTO3
#undef MBLS_MADC_UPTO2
#undef MBLS_MADC_UPTO1
#undef MBLS_MADC_UPTO0
#undef MBLS_MADC_CASE
#undef MBLS_MADC_REP14
#undef MBLS_MADC_REP13
#undef MBLS_MADC_REP12
#undef MBLS_MADC_REP11
#undef MBLS_MADC_REP10
#undef MBLS_MADC_REP9
#undef MBLS_MADC_REP8
#undef MBLS_MADC_REP7
#undef MBLS_MADC_REP6
#undef MBLS_MADC_REP5
#undef MBLS_MADC_REP4
#undef MBLS_MADC_REP3
#undef MBLS_MADC_REP2
#undef MBLS_MADC_REP1
#undef MBLS_MADC_REP0
#undef MBLS_MADC_SP
#undef MBLS_MADC_VP
#undef MBLS_MADC_SV
#undef MBLS_MADC_VT
#undef MBLS_MADC_ST

// acc: [+= tm tp, >>= SH (TAIL),] += sum va[i] vb[i] (NV terms) + sum sa[i] sb[i] (NS terms, sb
// compile-time constants), one chain in that order, in ceil(terms / MAXP) statements of equal length
template <bool TAIL, int SH, int NV, int NS>
MBLS_DEV void chain(uint64_t& acc, uint32_t tm, uint32_t tp, const uint32_t* va, const uint32_t* vb, const uint32_t* sa,
                    const uint32_t* sb) {
    constexpr int T = (TAIL ? 1 : 0) + NV + NS;
    if constexpr (T > 0) {
        constexpr int NST = (T + MAXP - 1) / MAXP, ROOM = (T + NST - 1) / NST - (TAIL ? 1 : 0);
        constexpr int nv = NV < ROOM ? NV : ROOM, ns = NS < ROOM - nv ? NS : ROOM - nv;
        stmt<TAIL, SH, nv, ns>(acc, tm, tp, va, vb, sa, sb);
        chain<false, SH, NV - nv, NS - ns>(acc, 0u, 0u, va + nv, vb + nv, sa + ns, sb + ns);
    }
}

// ta[j], tb[j] <- x[I + j], y[K - I - j] for i = I..HI: the terms of column K over that range
template <int K, int I, int HI, class X, class Y>
MBLS_DEV void fill(uint32_t* ta, uint32_t* tb, const X& x, const Y& y) {
#pragma unroll
    for (int j = 0; j <= HI - I; ++j) {
        ta[j] = x[I + j];
        tb[j] = y[K - I - j];
    }
}

// The split form: a column in statements of 8, 4, 2 and 1 mads, each writing a dummy SGPR pair for
// the carry-out.  Kept for the Fr product (mbls_fr29.hpp, inner.hip): the NTT pass runs 5 waves per
// SIMD, where another wave issues during a pad, and sits at its 96-register bound, where the packed
// form's longer statements cost it scratch (profiles/r08/README.md).
#define MBLS_MADC_STEP(A, B) "v_mad_u64_u32 %0, %1, " A ", " B ", %0\n\t"
#define MBLS_MADC_1 MBLS_MADC_STEP("%2", "%3")
#define MBLS_MADC_2 MBLS_MADC_1 MBLS_MADC_STEP("%4", "%5")
#define MBLS_MADC_4 MBLS_MADC_2 MBLS_MADC_STEP("%6", "%7") MBLS_MADC_STEP("%8", "%9")
#define MBLS_MADC_8                                                                                                  \
    MBLS_MADC_4 MBLS_MADC_STEP("%10", "%11") MBLS_MADC_STEP("%12", "%13") MBLS_MADC_STEP("%14", "%15") \
        MBLS_MADC_STEP("%16", "%17")

// acc += sum a_k b_k over N = 1, 2, 4, 8 pairs; S: the b operands are wave-uniform constants (SGPRs)
template <bool S>
MBLS_DEV void mad1(uint64_t& acc, uint32_t a0, uint32_t b0) {
    uint64_t c;
    if constexpr (S)
        asm(MBLS_MADC_1 : "+v"(acc), "=&s"(c) : "v"(a0), "s"(b0));
    else
        asm(MBLS_MADC_1 : "+v"(acc), "=&s"(c) : "v"(a0), "v"(b0));
}
template <bool S>
MBLS_DEV void mad2(uint64_t& acc, uint32_t a0, uint32_t b0, uint32_t a1, uint32_t b1) {
    uint64_t c;
    if constexpr (S)
        asm(MBLS_MADC_2 : "+v"(acc), "=&s"(c) : "v"(a0), "s"(b0), "v"(a1), "s"(b1));
    else
        asm(MBLS_MADC_2 : "+v"(acc), "=&s"(c) : "v"(a0), "v"(b0), "v"(a1), "v"(b1));
}
template <bool S>
MBLS_DEV void mad4(uint64_t& acc, uint32_t a0, uint32_t b0, uint32_t a1, uint32_t b1, uint32_t a2, uint32_t b2,
                   uint32_t a3, uint32_t b3) {
    uint64_t c;
    if constexpr (S)
        asm(MBLS_MADC_4 : "+v"(acc), "=&s"(c) : "v"(a0), "s"(b0), "v"(a1), "s"(b1), "v"(a2), "s"(b2), "v"(a3), "s"(b3));
    else
        asm(MBLS_MADC_4 : "+v"(acc), "=&s"(c) : "v"(a0), "v"(b0), "v"(a1), "v"(b1), "v"(a2), "v"(b2), "v"(a3), "v"(b3));
}
template <bool S>
MBLS_DEV void mad8(uint64_t& acc, uint32_t a0, uint32_t b0, uint32_t a1, uint32_t b1, uint32_t a2, uint32_t b2,
                   uint32_t a3, uint32_t b3, uint32_t a4, uint32_t b4, uint32_t a5, uint32_t b5, uint32_t a6,
                   uint32_t b6, uint32_t a7, uint32_t b7) {
    uint64_t c;
    if constexpr (S)
        asm(MBLS_MADC_8
            : "+v"(acc), "=&s"(c)
            : "v"(a0), "s"(b0), "v"(a1), "s"(b1), "v"(a2), "s"(b2), "v"(a3), "s"(b3), "v"(a4), "s"(b4), "v"(a5),
              "s"(b5), "v"(a6), "s"(b6), "v"(a7), "s"(b7));
    else
        asm(MBLS_MADC_8
            : "+v"(acc), "=&s"(c)
            : "v"(a0), "v"(b0), "v"(a1), "v"(b1), "v"(a2), "v"(b2), "v"(a3), "v"(b3), "v"(a4), "v"(b4), "v"(a5),
              "v"(b5), "v"(a6), "v"(b6), "v"(a7), "v"(b7));
}
#undef MBLS_MADC_8
#undef MBLS_MADC_4
#undef MBLS_MADC_2
#undef MBLS_MADC_1
#undef MBLS_MADC_STEP

// acc += sum_{i = I..HI} x[i] y[K - i] (S: y holds compile-time constants -> SGPR operands)
template <int K, int I, int HI, bool S, class X, class Y>
MBLS_DEV void col(uint64_t& acc, const X& x, const Y& y) {
    if constexpr (I <= HI) {
        constexpr int R = HI - I + 1;
        if constexpr (R >= 8) {
            mad8<S>(acc, x[I], y[K - I], x[I + 1], y[K - I - 1], x[I + 2], y[K - I - 2], x[I + 3], y[K - I - 3], x[I + 4],
                    y[K - I - 4], x[I + 5], y[K - I - 5], x[I + 6], y[K - I - 6], x[I + 7], y[K - I - 7]);
            col<K, I + 8, HI, S>(acc, x, y);
        } else if constexpr (R >= 4) {
            mad4<S>(acc, x[I], y[K - I], x[I + 1], y[K - I - 1], x[I + 2], y[K - I - 2], x[I + 3], y[K - I - 3]);
            col<K, I + 4, HI, S>(acc, x, y);
        } else if constexpr (R >= 2) {
            mad2<S>(acc, x[I], y[K - I], x[I + 1], y[K - I - 1]);
            col<K, I + 2, HI, S>(acc, x, y);
        } else {
            mad1<S>(acc, x[I], y[K - I]);
        }
    }
}

// Two independent columns (A, B) interleaved inside one statement: A0 B0 A1 B1 ... -- each chain's
// dependent mads are two instructions apart, so a wave waits half as long on the 64-bit mad
// latency (round 6: two products of a butterfly / an addition that do not depend on each other)
#define MBLS_MADX_STEP(ACC, A, B) "v_mad_u64_u32 " ACC ", %2, " A ", " B ", " ACC "\n\t"
template <bool S>
MBLS_DEV void madx1(uint64_t& p, uint64_t& q, uint32_t a0, uint32_t b0, uint32_t c0, uint32_t d0) {
    uint64_t c;
    if constexpr (S)
        asm(MBLS_MADX_STEP("%0", "%3", "%4") MBLS_MADX_STEP("%1", "%5", "%6")
            : "+v"(p), "+v"(q), "=&s"(c) : "v"(a0), "s"(b0), "v"(c0), "s"(d0));
    else
        asm(MBLS_MADX_STEP("%0", "%3", "%4") MBLS_MADX_STEP("%1", "%5", "%6")
            : "+v"(p), "+v"(q), "=&s"(c) : "v"(a0), "v"(b0), "v"(c0), "v"(d0));
}
template <bool S>
MBLS_DEV void madx4(uint64_t& p, uint64_t& q, uint32_t a0, uint32_t b0, uint32_t a1, uint32_t b1, uint32_t a2,
                    uint32_t b2, uint32_t a3, uint32_t b3, uint32_t c0, uint32_t d0, uint32_t c1, uint32_t d1,
                    uint32_t c2, uint32_t d2, uint32_t c3, uint32_t d3) {
    uint64_t c;
#define MBLS_MADX_4                                                                                                \
    MBLS_MADX_STEP("%0", "%3", "%4") MBLS_MADX_STEP("%1", "%11", "%12") MBLS_MADX_STEP("%0", "%5", "%6")             \
        MBLS_MADX_STEP("%1", "%13", "%14") MBLS_MADX_STEP("%0", "%7", "%8") MBLS_MADX_STEP("%1", "%15", "%16")       \
            MBLS_MADX_STEP("%0", "%9", "%10") MBLS_MADX_STEP("%1", "%17", "%18")
    if constexpr (S)
        asm(MBLS_MADX_4
            : "+v"(p), "+v"(q), "=&s"(c)
            : "v"(a0), "s"(b0), "v"(a1), "s"(b1), "v"(a2), "s"(b2), "v"(a3), "s"(b3), "v"(c0), "s"(d0), "v"(c1),
              "s"(d1), "v"(c2), "s"(d2), "v"(c3), "s"(d3));
    else
        asm(MBLS_MADX_4
            : "+v"(p), "+v"(q), "=&s"(c)
            : "v"(a0), "v"(b0), "v"(a1), "v"(b1), "v"(a2), "v"(b2), "v"(a3), "v"(b3), "v"(c0), "v"(d0), "v"(c1),
              "v"(d1), "v"(c2), "v"(d2), "v"(c3), "v"(d3));
#undef MBLS_MADX_4
}
#undef MBLS_MADX_STEP

// p += sum_{i = I..HI} x[i] y[K - i], q += the same over (u, v): one interleaved chain pair
template <int K, int I, int HI, bool S, class X, class Y>
MBLS_DEV void col2(uint64_t& p, const X& x, const Y& y, uint64_t& q, const X& u, const Y& v) {
    if constexpr (I <= HI) {
        constexpr int R = HI - I + 1;
        if constexpr (R >= 4) {
            madx4<S>(p, q, x[I], y[K - I], x[I + 1], y[K - I - 1], x[I + 2], y[K - I - 2], x[I + 3], y[K - I - 3], u[I],
                     v[K - I], u[I + 1], v[K - I - 1], u[I + 2], v[K - I - 2], u[I + 3], v[K - I - 3]);
            col2<K, I + 4, HI, S>(p, x, y, q, u, v);
        } else {
            madx1<S>(p, q, x[I], y[K - I], u[I], v[K - I]);
            col2<K, I + 1, HI, S>(p, x, y, q, u, v);
        }
    }
}

}  // namespace madc
}  // namespace mbls
