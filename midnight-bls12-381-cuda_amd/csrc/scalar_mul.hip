// scalar_mul.hip -- batch variable-base scalar multiplication, output[i] = scalars[i] * bases[i]
// (the reference declares bls12_381_g1_scalar_mul / _glv at point_ops.cu:1149 / :1019 behind
// GLV_ENABLED, which its build leaves off; it has no G2 form).  One lane per (scalar, point) pair.
//
// G1: s = +-m1 +- m2 lam (glv_split, m < 2^127) and phi(x, y) = (beta x, y) = [lam](x, y), so
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
//   The table lives in the leased scratch arena, 8 rows of 192 B per lane (a per-lane array
//   indexed by a run-time digit would go to scratch memory anyway; in LDS 64 lanes x 768 B of
//   affine rows would cap a CU at three waves): each lane writes and reads only its own rows, so
//   no barrier is needed.
// G2: s = sum_j +-m_j psi^j(P) (psi_split, m_j < 2^63) on the generic Jacobian<Fq2>: the signs
//   go into the four affine images, the 15 non-empty subset sums of the images form a table
//   (Straus), and one chain of 63 doublings adds the entry the four bits of a step select.
// Not constant time: branches and table addresses depend on the scalar's digits.
// Inputs are assumed to lie in the order-r subgroup (the splits use [lam] = phi, [z] = psi).
#include <hip/hip_runtime.h>

#include "mbls_common.hpp"
#include "mbls_curve.hpp"
#include "mbls_fq28.hpp"
#include "mbls_split.hpp"

namespace mbls {

static constexpr int SM_MAX_BATCH = 1 << 26;  // point_ops.cu:745 MAX_POINT_BATCH_SIZE
static constexpr int SM_BLOCK = 64;           // one wave per workgroup: no LDS, no barriers
static constexpr int SM_G1_ROWS = 8;          // [1..8] P
static constexpr int SM_G1_ROW = 192;         // bytes: (X, Y, Z, Z prefix) while built, then affine (x, y)
static constexpr int SM_G2_ROWS = 15;         // non-empty subsets of {+-psi^j P}
// lanes per launch: bounds the table (G1 384 MiB, G2 270 MiB) whatever the batch size
static constexpr size_t SM_G1_CHUNK = (size_t)1 << 18;
static constexpr size_t SM_G2_CHUNK = (size_t)1 << 16;

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

}  // namespace sm

template <bool MONT>
__global__ __launch_bounds__(SM_BLOCK) void k_scalar_mul_g1(const uint8_t* __restrict__ bases,
                                                            const uint8_t* __restrict__ scalars,
                                                            uint8_t* __restrict__ out, uint8_t* __restrict__ tbl,
                                                            uint32_t n) {
    using namespace r28;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<Fq> b = load_affine<Fq>(bases, i);
    uint8_t* o = out + (size_t)i * 144;
    if (b.is_inf()) {
        sm::store_j28(o, J28::inf());
        return;
    }
    uint8_t* T = tbl + (size_t)i * (SM_G1_ROWS * SM_G1_ROW);
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
            sm::store_j28(r, acc);
            sm::st28(r + 144, pz);
            pz = mul(pz, acc.z);
        }
        Fq w;
        to_words(pz, w.v);
        w = inv(w);  // (v R)^-1 R^2 = v^-1 R; unpack_shift8 makes it v^-1 R'
        F28 ia = unpack_shift8(w.v);
#pragma unroll 1
        for (int e = SM_G1_ROWS - 1; e > 0; --e) {
            uint8_t* r = T + e * SM_G1_ROW;
            const F28 zi = mul(ia, sm::ld28(r + 144));  // 1 / Z_e
            ia = mul(ia, sm::ld28(r + 96));             // 1 / (Z_1 ... Z_(e-1))
            const F28 zi2 = sqr(zi);
            const F28 x = mul(sm::ld28(r), zi2), y = mul(mul(sm::ld28(r + 48), zi2), zi);
            sm::st28(r, x);
            sm::st28(r + 48, y);
        }
    }
    uint32_t m0[4], m1[4];
    bool neg0, neg1;
    glv_split(load_scalar<MONT>(scalars, i), m0, neg0, m1, neg1);
    sm::add_eights(m0);
    sm::add_eights(m1);
    Fq bw;
#pragma unroll
    for (int k = 0; k < 12; ++k) bw.v[k] = GLV_BETA_MONT[k];
    const F28 beta = unpack_shift8(bw.v);
    acc = J28::inf();
#pragma unroll 1
    for (int w = 0; w < 32; ++w) {
        if (!acc.is_inf()) {
#pragma unroll 1
            for (int k = 0; k < 4; ++k) acc = dbl(acc);
        }
        const int d0 = sm::pop_digit(m0), d1 = sm::pop_digit(m1);
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
    sm::store_j28(o, acc);
}

template <bool MONT>
__global__ __launch_bounds__(SM_BLOCK) void k_scalar_mul_g2(const uint8_t* __restrict__ bases,
                                                            const uint8_t* __restrict__ scalars,
                                                            uint8_t* __restrict__ out, uint8_t* __restrict__ tbl,
                                                            uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<Fq2> q0 = load_affine<Fq2>(bases, i), q1, q2, q3;
    if (q0.is_inf()) {
        store_jac<Fq2>(out, i, Jacobian<Fq2>::inf());
        return;
    }
    uint64_t m[4];
    bool ng[4];
    psi_split(load_scalar<MONT>(scalars, i), m, ng);
    psi_images(q0, q1, q2, q3);
    if (ng[0]) q0.y = neg(q0.y);
    if (ng[1]) q1.y = neg(q1.y);
    if (ng[2]) q2.y = neg(q2.y);
    if (ng[3]) q3.y = neg(q3.y);
    // row k - 1 = sum of the images whose bit is set in k: the four images first, then every
    // other k from the rows of its lowest bit and of the rest (both already written)
    uint8_t* T = tbl + (size_t)i * (SM_G2_ROWS * 288);
    store_jac<Fq2>(T, 0, Jacobian<Fq2>::from_affine(q0));
    store_jac<Fq2>(T, 1, Jacobian<Fq2>::from_affine(q1));
    store_jac<Fq2>(T, 3, Jacobian<Fq2>::from_affine(q2));
    store_jac<Fq2>(T, 7, Jacobian<Fq2>::from_affine(q3));
#pragma unroll 1
    for (uint32_t k = 3; k <= SM_G2_ROWS; ++k) {
        const uint32_t low = k & (0u - k), rest = k ^ low;
        if (rest == 0) continue;
        store_jac<Fq2>(T, k - 1, jac_add(load_jac<Fq2>(T, rest - 1), load_jac<Fq2>(T, low - 1)));
    }
    Jacobian<Fq2> acc = Jacobian<Fq2>::inf();
#pragma unroll 1
    for (int bit = 62; bit >= 0; --bit) {  // m_j < 2^63
        acc = jac_dbl(acc);
        const uint32_t k = (uint32_t)((m[0] >> bit) & 1) | (uint32_t)((m[1] >> bit) & 1) << 1 |
                           (uint32_t)((m[2] >> bit) & 1) << 2 | (uint32_t)((m[3] >> bit) & 1) << 3;
        if (k) acc = jac_add(acc, load_jac<Fq2>(T, k - 1));
    }
    store_jac<Fq2>(out, i, acc);
}

// placement as the reference (point_ops.cu:1044-1046): is_a_on_device the bases, is_b_on_device
// the scalars, is_result_on_device the output; host buffers go through the leased arena
template <bool G2>
static eIcicleError scalar_mul_call(const void* bases, const void* scalars, int size, bool mont,
                                    const VecOpsConfig* cfg, void* output) {
    // point_ops.cu:1027-1035
    if (!bases || !scalars || !output || !cfg) return MBLS_INVALID_ARGUMENT;
    if (size <= 0 || size > SM_MAX_BATCH) return MBLS_INVALID_ARGUMENT;
    using PS = PointSize<typename std::conditional<G2, Fq2, Fq>::type>;
    constexpr size_t AFF = PS::AFF, JAC = PS::JAC;
    constexpr size_t ROW = G2 ? SM_G2_ROWS * JAC : SM_G1_ROWS * SM_G1_ROW, CHUNK = G2 ? SM_G2_CHUNK : SM_G1_CHUNK;
    const size_t n = (size_t)size;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *tbl, *dout;
    const uint8_t *db, *ds;
    S.scratch(&tbl, (n < CHUNK ? n : CHUNK) * ROW);
    S.in(&db, bases, n * AFF, cfg->is_a_on_device);
    S.in(&ds, scalars, n * 32, cfg->is_b_on_device);
    S.out(&dout, output, n * JAC, cfg->is_result_on_device);
    const eIcicleError er = S.open();
    if (er != MBLS_SUCCESS) return er;
    {
        ProfScope prof(G2 ? "scalar_mul.g2" : "scalar_mul.g1", st);
        for (size_t i0 = 0; i0 < n; i0 += CHUNK) {  // stream order serialises the chunks on the table
            const uint32_t cn = (uint32_t)(n - i0 < CHUNK ? n - i0 : CHUNK);
            const dim3 grid((cn + SM_BLOCK - 1) / SM_BLOCK), block(SM_BLOCK);
            const uint8_t *cb = db + i0 * AFF, *cs = ds + i0 * 32;
            uint8_t* co = dout + i0 * JAC;
            if (G2) {
                if (mont)
                    hipLaunchKernelGGL(k_scalar_mul_g2<true>, grid, block, 0, st, cb, cs, co, tbl, cn);
                else
                    hipLaunchKernelGGL(k_scalar_mul_g2<false>, grid, block, 0, st, cb, cs, co, tbl, cn);
            } else {
                if (mont)
                    hipLaunchKernelGGL(k_scalar_mul_g1<true>, grid, block, 0, st, cb, cs, co, tbl, cn);
                else
                    hipLaunchKernelGGL(k_scalar_mul_g1<false>, grid, block, 0, st, cb, cs, co, tbl, cn);
            }
            MBLS_TRY(hipGetLastError());
        }
    }
    return S.close(cfg->is_async);
}

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError bls12_381_g1_scalar_mul(const mbls_g1_affine_t* bases, const mbls_fr_t* scalars, int size,
                                     const VecOpsConfig* config, mbls_g1_projective_t* output) {
    return scalar_mul_call<false>(bases, scalars, size, false, config, output);
}
eIcicleError bls12_381_g1_scalar_mul_glv(const mbls_g1_affine_t* bases, const mbls_fr_t* scalars, int size,
                                         const VecOpsConfig* config, mbls_g1_projective_t* output) {
    return scalar_mul_call<false>(bases, scalars, size, false, config, output);
}
eIcicleError bls12_381_g2_scalar_mul(const mbls_g2_affine_t* bases, const mbls_fr_t* scalars, int size,
                                     const VecOpsConfig* config, mbls_g2_projective_t* output) {
    return scalar_mul_call<true>(bases, scalars, size, false, config, output);
}
eIcicleError mbls_g1_scalar_mul(const mbls_g1_affine_t* bases, const mbls_fr_t* scalars, int size,
                                bool scalars_montgomery, const VecOpsConfig* config, mbls_g1_projective_t* output) {
    return scalar_mul_call<false>(bases, scalars, size, scalars_montgomery, config, output);
}
eIcicleError mbls_g2_scalar_mul(const mbls_g2_affine_t* bases, const mbls_fr_t* scalars, int size,
                                bool scalars_montgomery, const VecOpsConfig* config, mbls_g2_projective_t* output) {
    return scalar_mul_call<true>(bases, scalars, size, scalars_montgomery, config, output);
}

}  // extern "C"
