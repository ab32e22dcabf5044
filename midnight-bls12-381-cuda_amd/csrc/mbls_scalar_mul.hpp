// mbls_scalar_mul.hpp -- the G1 GLV scalar multiplication of one lane, shared by the batch scalar
// multiplication (scalar_mul.hip) and the EC-NTT's butterflies (ecntt.hip).  Device only.
//
// s = +-m1 +- m2 lam (glv_split, m < 2^127) and phi(x, y) = (beta x, y) = [lam](x, y), so
//   s P = sum_w 16^w (d1_w P + d2_w phi(P)): ONE chain of 31 x 4 doublings shared by both halves,
//   signed 4-bit digits d in [-8, 7] (digit w = nibble w of m + 0x88..8, minus 8: no carry to
//   track, and m + 0x88..8 < 2^128 because m <= lam / 2 + 1 < 0x57 2^120) against one table
//   [1..8] P.  phi of a table entry is one product of its x by beta, the sign negates its y.
//   The table is AFFINE behind one inversion per lane (Montgomery's trick over the seven Z's), so
//   every addition of the chain is the mixed madd (6M + 3S + mul2 against jadd's 10M + 4S + mul2):
//   measured 26.7 ms against 29.2 ms with a Jacobian table at n = 2^20.
//   Arithmetic: the radix-2^28 lane types (mbls_fq28.hpp) inside their documented bounds -- the
//   accumulator keeps J28's invariant (dbl and madd each restore it), table entries are
//   canonical words read back through unpack_shift8 (normalised, < 256 p), y is negated on the
//   canonical words (p - y, still canonical) and beta x is a product of two unpacked values:
//   normalised and < p (1 + 2^16 p / 2^392) < 33 p, inside madd's < 256 p.  The table's own
//   products (Z prefixes, 1 / Z, x / Z^2, y / Z^3) multiply normalised operands only.
//   The table lives in the caller's scratch, 8 rows of 192 B per lane (a per-lane array
//   indexed by a run-time digit would go to scratch memory anyway; in LDS 64 lanes x 768 B of
//   affine rows would cap a CU at three waves): each lane writes and reads only its own rows, so
//   no barrier is needed.
// Not constant time: branches and table addresses depend on the scalar's digits.
// The point is assumed to lie in the order-r subgroup (the split uses [lam] = phi).
#pragma once
#include "mbls_curve.hpp"
#include "mbls_fq28.hpp"
#include "mbls_split.hpp"

namespace mbls {

static constexpr int SM_BLOCK = 64;    // one wave per workgroup: no LDS, no barriers
static constexpr int SM_G1_ROWS = 8;   // [1..8] P
static constexpr int SM_G1_ROW = 192;  // bytes: (X, Y, Z, Z prefix) while built, then affine (x, y)
// lanes per launch: bounds the G1 table (384 MiB) whatever the batch size
static constexpr size_t SM_G1_CHUNK = (size_t)1 << 18;

namespace sm {
using namespace r28;

MBLS_DEV F28 ld28(const uint8_t* p) {
    const Fq w = load<FqCfg>(p);
    return unpack_shift8(w.v);
}
MBLS_DEV void st28(uint8_t* p, const F28& a) {
    Fq w;
    to_words(a, w.v);
    store<FqCfg>(p, w);
}
MBLS_DEV void store_j28(uint8_t* p, const J28& a) {
    st28(p, a.x);
    st28(p + 48, a.y);
    st28(p + 96, a.z);
}

MBLS_DEV void add_eights(uint32_t (&m)[4]) {  // m + 0x8888...8 (no carry out: see the header)
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = __builtin_addc(m[k], 0x88888888u, c, &c);
}
MBLS_DEV int pop_digit(uint32_t (&m)[4]) {  // top nibble - 8; m <<= 4
    const int d = (int)(m[3] >> 28) - 8;
#pragma unroll
    for (int k = 3; k > 0; --k) m[k] = (m[k] << 4) | (m[k - 1] >> 28);
    m[0] <<= 4;
    return d;
}

// [scalars[si]] b for an affine b that is not the identity; T: this lane's SM_G1_ROWS rows of
// SM_G1_ROW bytes.  The scalar is read only once the table stands (its words would otherwise
// live across the table's products).
template <bool MONT>
MBLS_DEV J28 g1_glv_mul(const Affine<Fq>& b, const uint8_t* __restrict__ scalars, size_t si, uint8_t* T) {
    J28 acc = J28::inf();
    {
        // [1..8] P by repeated mixed addition: the first step takes madd's identity branch, the
        // second its P == Q branch (dbl).  Row 0 is P itself; rows 1..7 are parked as (X, Y, Z,
        // product of the Z's before this row) and made affine behind ONE inversion (Montgomery's
        // trick, as k_jac_to_affine).  Every operand below is normalised (a product, or words
        // through unpack_shift8) except acc.z (limbs < 2^29, J28's invariant) against the
        // normalised prefix: 14 * 2^57 + 14 * 2^56, inside mul's column bound.
        store<FqCfg>(T, b.x);
        store<FqCfg>(T + 48, b.y);
        const F28 px = unpack_shift8(b.x.v), py = unpack_shift8(b.y.v);
        F28 pz = F28::one();
#pragma unroll 1
        for (int e = 0; e < SM_G1_ROWS; ++e) {
            madd(acc, px, py);
            if (e == 0) continue;
            uint8_t* r = T + e * SM_G1_ROW;
            store_j28(r, acc);
            st28(r + 144, pz);
            pz = mul(pz, acc.z);
        }
        Fq w;
        to_words(pz, w.v);
        w = inv(w);  // (v R)^-1 R^2 = v^-1 R; unpack_shift8 makes it v^-1 R'
        F28 ia = unpack_shift8(w.v);
#pragma unroll 1
        for (int e = SM_G1_ROWS - 1; e > 0; --e) {
            uint8_t* r = T + e * SM_G1_ROW;
            const F28 zi = mul(ia, ld28(r + 144));  // 1 / Z_e
            ia = mul(ia, ld28(r + 96));             // 1 / (Z_1 ... Z_(e-1))
            const F28 zi2 = sqr(zi);
            const F28 x = mul(ld28(r), zi2), y = mul(mul(ld28(r + 48), zi2), zi);
            st28(r, x);
            st28(r + 48, y);
        }
    }
    uint32_t m0[4], m1[4];
    bool neg0, neg1;
    glv_split(load_scalar<MONT>(scalars, si), m0, neg0, m1, neg1);
    add_eights(m0);
    add_eights(m1);
    const F28 beta = unpack_shift8(glv_beta().v);
    acc = J28::inf();
#pragma unroll 1
    for (int w = 0; w < 32; ++w) {
        if (!acc.is_inf()) {
#pragma unroll 1
            for (int k = 0; k < 4; ++k) acc = dbl(acc);
        }
        const int d0 = pop_digit(m0), d1 = pop_digit(m1);
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {  // one madd site
            const int d = h ? d1 : d0;
            if (d == 0) continue;
            const bool ng = (h ? neg1 : neg0) != (d < 0);
            const uint8_t* q = T + ((d < 0 ? -d : d) - 1) * SM_G1_ROW;
            const Fq qx = load<FqCfg>(q);
            Fq qy = load<FqCfg>(q + 48);
            if (ng) qy = neg(qy);
            F28 x = unpack_shift8(qx.v);
            if (h) x = mul(x, beta);
            madd(acc, x, unpack_shift8(qy.v));
        }
    }
    return acc;
}

}  // namespace sm
}  // namespace mbls
