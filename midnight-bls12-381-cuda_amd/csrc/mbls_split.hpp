// mbls_split.hpp -- scalar loading and the endomorphism splits shared by the MSM front end
// (msm_common.hip) and the batch scalar multiplication (scalar_mul.hip): reduction of standard
// scalars, the G1 GLV split with the phi constant, the G2 four-way psi split with the psi images.
// Device only; the constants have internal linkage so every translation unit carries its own copy.
#pragma once
#include "mbls_curve.hpp"

namespace mbls {

// ------------------------------------------------------------------------------------
// 0. scalars.  The reference's raw entry digitises all 256 bits of a standard-form scalar
//    (msm_kernels.cu:86-142, W = ceil(256 / c) at :648), so ANY 32-byte s gives s P; on the
//    order-r subgroup that is (s mod r) P.  The GLV / psi splits and the closed-form digits
//    assume s < r, so standard scalars are reduced first: 2^256 < 3r, two conditional
//    subtractions (tests/test_gpu_parity.py::test_msm_noncanonical_scalars).
//    Montgomery scalars need none: from_mont of any 256-bit word string is already < r.
// ------------------------------------------------------------------------------------
MBLS_DEV void reduce_scalar_words(uint32_t (&x)[8]) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        uint32_t t[8];
        const uint32_t borrow = sub_mod_raw<FrCfg>(t, x);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = borrow ? x[i] : t[i];
    }
}
template <bool MONT>
MBLS_DEV Fr load_scalar(const uint8_t* __restrict__ scalars, size_t i) {
    Fr s = load<FrCfg>(scalars + 32 * i);
    if (MONT)
        s = from_mont(s);
    else
        reduce_scalar_words(s.v);
    return s;
}

// ------------------------------------------------------------------------------------
// GLV split (G1): s = +-m1 +- m2*lam (mod r), m1, m2 < 2^127 (oracle/pyref.py
// glv_decompose), lam = z^2 - 1 and r = lam^2 + lam + 1.
// ------------------------------------------------------------------------------------
static __constant__ uint32_t GLV_LAM[4] = {0xffffffffu, 0x00000000u, 0x0001a402u, 0xac45a401u};
static __constant__ uint32_t GLV_HALF[4] = {0x7fffffffu, 0x00000000u, 0x8000d201u, 0x5622d200u};
// floor(2^383 / lam)
static __constant__ uint32_t GLV_G[8] = {0xc4b6396eu, 0xed2f27c6u, 0x9345fbd1u, 0x1c4fa4d3u,
                                         0x7b67f718u, 0xb1fb7291u, 0xf00fd56eu, 0xbe35f678u};

MBLS_DEV bool gt4(const uint32_t* a, const uint32_t* b) {  // a > b, 4 words
    bool gt = false, eq = true;
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        gt = gt || (eq && a[k] > b[k]);
        eq = eq && a[k] == b[k];
    }
    return gt;
}
MBLS_DEV void sub4(uint32_t* d, const uint32_t* a, const uint32_t* b) {  // d = a - b
    uint64_t br = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint64_t t = (uint64_t)a[k] - b[k] - br;
        d[k] = (uint32_t)t;
        br = (t >> 63) & 1;
    }
}
MBLS_DEV void add4_u32(uint32_t* a, uint32_t x) {
    uint64_t c = x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint64_t t = (uint64_t)a[k] + c;
        a[k] = (uint32_t)t;
        c = t >> 32;
    }
}
MBLS_DEV void sub4_u32(uint32_t* a, uint32_t x) {
    uint64_t br = x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint64_t t = (uint64_t)a[k] - br;
        a[k] = (uint32_t)t;
        br = (t >> 63) & 1;
    }
}

MBLS_DEV void glv_split(const Fr& s, uint32_t (&m1)[4], bool& neg1, uint32_t (&m2)[4], bool& neg2) {
    // q_est = floor(s * G / 2^383) in {q - 1, q}
    uint32_t prod[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) prod[k] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint64_t t = (uint64_t)s.v[i] * GLV_G[j] + prod[i + j] + c;
            prod[i + j] = (uint32_t)t;
            c = t >> 32;
        }
        prod[i + 8] = (uint32_t)c;
    }
    uint32_t q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = (prod[11 + k] >> 31) | (prod[12 + k] << 1);
    // rem = s - q * lam  (< 2 lam < 2^129)
    uint32_t ql[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) ql[k] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint64_t t = (uint64_t)q[i] * GLV_LAM[j] + ql[i + j] + c;
            ql[i + j] = (uint32_t)t;
            c = t >> 32;
        }
        ql[i + 4] = (uint32_t)c;
    }
    uint32_t rem[5];
    {
        uint64_t br = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            uint64_t t = (uint64_t)s.v[k] - ql[k] - br;
            rem[k] = (uint32_t)t;
            br = (t >> 63) & 1;
        }
    }
    uint32_t k1[4] = {rem[0], rem[1], rem[2], rem[3]};
    if (rem[4] != 0 || !gt4(GLV_LAM, k1)) {  // rem >= lam
        sub4(k1, k1, GLV_LAM);
        add4_u32(q, 1);
    }
    // balance k1 into (-lam/2, lam/2]
    neg1 = gt4(k1, GLV_HALF);
    if (neg1) {
        sub4(m1, GLV_LAM, k1);
        add4_u32(q, 1);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) m1[k] = k1[k];
    }
    // balance k2: (k2 - lam - 1) * lam == k2 * lam + 1 (mod r), so k1 absorbs a -1
    neg2 = gt4(q, GLV_HALF);
    if (neg2) {
        sub4(m2, GLV_LAM, q);
        add4_u32(m2, 1);
        if (neg1) {
            add4_u32(m1, 1);
        } else if ((m1[0] | m1[1] | m1[2] | m1[3]) == 0) {
            m1[0] = 1;
            neg1 = true;
        } else {
            sub4_u32(m1, 1);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) m2[k] = q[k];
    }
}

// phi(x, y) = (beta x, y) (Montgomery); identity (0, 0) maps to itself.
// beta: the cube root of unity in Fq with phi(G) = lam G (oracle/pyref.py GLV_BETA)
static __constant__ uint32_t GLV_BETA_MONT[12] = {0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u,
                                                  0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu,
                                                  0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u};
MBLS_DEV Fq glv_beta() {
    Fq beta;
#pragma unroll
    for (int k = 0; k < 12; ++k) beta.v[k] = GLV_BETA_MONT[k];
    return beta;
}

// ------------------------------------------------------------------------------------
// psi split (G2): s == sum_j (-1)^neg_j m_j psi^j(Q) on G2, m_j < 2^63
//      (oracle/pyref.py psi_decompose).  psi = [z] on G2 and r = x^4 - x^2 + 1 for x = |z|,
//      so balanced base-x digits d_j (|d_j| <= x/2) plus the carry d_4 folded back with
//      x^4 == x^2 - 1 give s == sum_j d_j x^j == sum_j (-1)^j d_j z^j.
// ------------------------------------------------------------------------------------
static constexpr uint64_t PSI_X = 0xd201000000010000ull;  // |z| = PSI_XP << 16
static constexpr uint64_t PSI_XP = 0xd20100000001ull;

// t <- t div |z|, returns t mod |z|  (t: 8 little-endian u32 words).  |z| = 2^16 x' with a
// 48-bit x', so the division is a 16-bit-digit long division of t >> 16 by x' (every partial
// remainder * 2^16 + digit fits 64 bits).
MBLS_DEV uint64_t divmod_x(uint32_t (&t)[8]) {
    const uint32_t low16 = t[0] & 0xffffu;
    uint64_t r = 0;
    uint32_t q[8];
#pragma unroll
    for (int w = 7; w >= 0; --w) {
        const uint32_t uw = (t[w] >> 16) | (w < 7 ? (t[w + 1] << 16) : 0u);  // word w of t >> 16
        uint64_t cur = (r << 16) | (uw >> 16);
        const uint64_t qh = cur / PSI_XP;
        r = cur - qh * PSI_XP;
        cur = (r << 16) | (uw & 0xffffu);
        const uint64_t ql = cur / PSI_XP;
        r = cur - ql * PSI_XP;
        q[w] = (uint32_t)((qh << 16) | ql);
    }
#pragma unroll
    for (int w = 0; w < 8; ++w) t[w] = q[w];
    return (r << 16) | low16;
}

// the four digits of a reduced scalar (s < r): magnitude m[j] with neg[j] the sign against psi^j
MBLS_DEV void psi_split(const Fr& s, uint64_t (&m)[4], bool (&neg)[4]) {
    uint32_t t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = s.v[k];
    int64_t d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t rem = divmod_x(t);
        if (rem > (PSI_X >> 1)) {  // balance: rem - x, carry one into the quotient
            d[j] = -(int64_t)(PSI_X - rem);
            unsigned c = 1;
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = __builtin_addc(t[k], 0u, c, &c);
        } else {
            d[j] = (int64_t)rem;
        }
    }
    const int64_t d4 = (int64_t)t[0];  // s < r < x^4: the fifth digit is 0 or 1
    d[2] += d4;
    d[0] -= d4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        neg[j] = (d[j] < 0) != ((j & 1) != 0);  // psi^j = [z^j] = [(-x)^j]
        m[j] = (uint64_t)(d[j] < 0 ? -d[j] : d[j]);
    }
}

// psi(x, y) = (conj(x) * CX, conj(y) * CY), CX = (0, CX1) (oracle/pyref.py PSI_CX / PSI_CY),
// Montgomery limbs
// psi^2 x-multiplier C2 = 0x1a0111ea...00000000aaac (an Fq cube root of unity), Montgomery form
static __constant__ uint32_t PSI2_CX_MONT[12] = {0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u,
                                                 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu,
                                                 0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u};
static __constant__ uint32_t PSI_CX1_MONT[12] = {0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u,
                                                 0x309b7e2cu, 0x50880866u, 0x7e881024u, 0xa20d1b8cu,
                                                 0xe2db9068u, 0x14e4f04fu, 0x1564853au, 0x14e56d3fu};
static __constant__ uint32_t PSI_CY0_MONT[12] = {0xa55c9ad1u, 0x3e2f585du, 0x86c18183u, 0x4294213du,
                                                 0x8b623732u, 0x382844c8u, 0x19103e18u, 0x92ad2afdu,
                                                 0xac7cf0b9u, 0x1d794e4fu, 0x7d825ec8u, 0x0bd592fcu};
static __constant__ uint32_t PSI_CY1_MONT[12] = {0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u,
                                                 0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u,
                                                 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu};

// psi(P) alone, of a pair-sliced point (mbls_pairfield.hpp: lane 2k holds c0, lane 2k+1 c1): the
// field values psi_images gives q1, Montgomery; identity (0, 0) maps to itself.  The subgroup test
// of check_points.hip compares it with [z] P.
MBLS_DEV Affine<PFq2> psi_image(const Affine<PFq2>& p) {
    const bool j = pairdpp::odd();
    Fq cx1, cy;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        cx1.v[k] = PSI_CX1_MONT[k];
        cy.v[k] = j ? PSI_CY1_MONT[k] : PSI_CY0_MONT[k];
    }
    Affine<PFq2> q;
    q.x = PFq2{partner(p.x.v) * cx1};                                // x1 CX1 + x0 CX1 u
    q.y = PFq2{select(j, neg(p.y.v), p.y.v)} * PFq2{cy};             // conj(y) * CY
    return q;
}

// psi(P), psi^2(P), psi^3(P) of one G2 point, Montgomery
MBLS_DEV void psi_images(const Affine<Fq2>& p, Affine<Fq2>& q1, Affine<Fq2>& q2, Affine<Fq2>& q3) {
    Fq cx1;
    Fq2 cy;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        cx1.v[k] = PSI_CX1_MONT[k];
        cy.c0.v[k] = PSI_CY0_MONT[k];
        cy.c1.v[k] = PSI_CY1_MONT[k];
    }
    // psi(P): conj(x) * (CX1 u) = x1 CX1 + x0 CX1 u, conj(y) * CY (5 Fq products); identity
    // (0, 0) maps to itself
    q1.x.c0 = p.x.c1 * cx1;
    q1.x.c1 = p.x.c0 * cx1;
    {  // conj(y) * CY, Karatsuba in line (fq2_mul is out of line: a call frame in scratch)
        const Fq a0 = p.y.c0, a1 = neg(p.y.c1);
        const Fq t0 = a0 * cy.c0, t1 = a1 * cy.c1, t2 = (a0 + a1) * (cy.c0 + cy.c1);
        q1.y = Fq2{t0 - t1, (t2 - t0) - t1};
    }
    // psi^2 = (x, y) -> (C2 x, -y) with C2 in Fq (oracle/pyref.py psi, checked numerically),
    // so psi^2(P) and psi^3(P) = psi^2(psi(P)) take 2 Fq products each (15 -> 9 per point)
    Fq c2;
#pragma unroll
    for (int k = 0; k < 12; ++k) c2.v[k] = PSI2_CX_MONT[k];
    q2 = Affine<Fq2>{Fq2{p.x.c0 * c2, p.x.c1 * c2}, neg(p.y)};
    q3 = Affine<Fq2>{Fq2{q1.x.c0 * c2, q1.x.c1 * c2}, neg(q1.y)};
}

}  // namespace mbls
