// scalar_mul.hip -- batch variable-base scalar multiplication, output[i] = scalars[i] * bases[i]
// (the reference declares bls12_381_g1_scalar_mul / _glv at point_ops.cu:1149 / :1019 behind
// GLV_ENABLED, which its build leaves off; it has no G2 form).  One lane per (scalar, point) pair.
//
// G1: the GLV multiplication of mbls_scalar_mul.hpp (sm::g1_glv_mul: signed 4-bit digits of both
//   halves against one affine table [1..8] P in the leased scratch arena, one shared doubling
//   chain), which the EC-NTT's butterflies (ecntt.hip) run too.
// G2: s = sum_j +-m_j psi^j(P) (psi_split, m_j < 2^63) on the generic Jacobian<Fq2>: the signs
//   go into the four affine images, the 15 non-empty subset sums of the images form a table
//   (Straus), and one chain of 63 doublings adds the entry the four bits of a step select.
// Not constant time: branches and table addresses depend on the scalar's digits.
// Inputs are assumed to lie in the order-r subgroup (the splits use [lam] = phi, [z] = psi).
#include <hip/hip_runtime.h>

#include "mbls_common.hpp"
#include "mbls_curve.hpp"
#include "mbls_scalar_mul.hpp"

namespace mbls {

static constexpr int SM_MAX_BATCH = 1 << 26;  // point_ops.cu:745 MAX_POINT_BATCH_SIZE
static constexpr int SM_G2_ROWS = 15;  // non-empty subsets of {+-psi^j P}
// lanes per launch: bounds the G2 table (270 MiB) whatever the batch size (G1: SM_G1_CHUNK)
static constexpr size_t SM_G2_CHUNK = (size_t)1 << 16;

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
    sm::store_j28(o, sm::g1_glv_mul<MONT>(b, scalars, i, tbl + (size_t)i * (SM_G1_ROWS * SM_G1_ROW)));
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
