// ecntt.hip -- G1 EC-NTT (mbls_g1_ecntt): the NTT's butterflies over G1 points, scalars = the
// canonical roots of unity.  forward out_j = sum_i [w^(ij)] P_i, inverse out_i = [n^-1] sum_j
// [w^(-ij)] P_j, w = ROOT_OF_UNITY^(2^(32-k)) for n = 2^k, natural order in and out: the inverse
// of a monomial KZG SRS [s^j] G is the Lagrange SRS [L_i(s)] G (the reference's g_to_lagrange,
// which it runs on the CPU; it has no device form).
//
// Radix-2 decimation in time over an AFFINE work array W in the leased arena:
//   twiddles  k_ecntt_twiddles: w^(+-i), i < n/2, and n^-1 in slot n/2, one exponentiation per
//             entry, stored as standard-form 32-byte scalars (what the GLV split reads).
//   way in    forward: k_ecntt_gather, W[i] = in[bitrev i].  inverse: k_ecntt_scale, one lane per
//             point, J[i] = [n^-1] in[bitrev i] (the transform is linear, and stage 1 has no other
//             multiplication to fold the factor into), then the normalisation J -> W.
//   stage s   k_ecntt_stage, one lane per butterfly (a, b) = (W[ia], W[ia + 2^(s-1)]): t = [tw] b
//             with the G1 GLV body of mbls_scalar_mul.hpp, J[ia] = t + a, J[ib] = -(t + (-a)), both
//             by the mixed madd against the affine a.  A lane whose twiddle is 1 (j = 0 of every
//             block, all of stage 1) skips the multiplication, a lane whose b is the identity
//             stores a twice, a lane whose a is the identity stores t and -t.
//   normalise k_jac_to_affine<Fq> (points.hip) J -> W after every stage, into the output after the
//             last: the output is canonical affine.
//   Launches carry at most SM_G1_CHUNK lanes, so the table [1..8] b stays below 384 MiB; stream
//   order serialises the launches of a stage on it.  input == output is allowed: the input is
//   only read on the way in, the output only written by the last normalisation.
// Multiplications: forward (n/2) k - (n - 1) (stage s has 2^(k-s) blocks whose j = 0 is free),
// inverse n more.
//
// Limb bounds (mbls_fq28.hpp).  t leaves g1_glv_mul, or madd's identity branch on b's unpacked
// words, with J28's invariant.  madd's affine operand is a from the work array: canonical words
// through unpack_shift8 (normalised, < 256 p), its y negated on the canonical words for the
// difference (p - y, still canonical).  Each madd restores the invariant, so store_j28 (to_words:
// any value < 2^391) writes canonical words; the difference's Y is negated on those words.  The
// exceptional cases a = +-t take madd's own doubling and identity branches.
// Not constant time (the scalars are public roots of unity).  Inputs are assumed to lie in the
// order-r subgroup (the GLV split uses [lam] = phi).
#include <hip/hip_runtime.h>
#include <string.h>

#include "mbls_common.hpp"
#include "mbls_curve.hpp"
#include "mbls_scalar_mul.hpp"

namespace mbls {

static constexpr int ECNTT_MAX_LOG = 26;  // sizes up to 2^26, as the batch point entries

MBLS_DEV uint32_t ecntt_bitrev(uint32_t x, int bits) {
    return bits == 0 ? 0u : (__builtin_bitreverse32(x) >> (32 - bits));
}

// tw[i] = w^i for i < half, tw[half] = n_inv; w and n_inv Montgomery, the table standard form
__global__ void k_ecntt_twiddles(uint8_t* __restrict__ tw, Fr w, Fr n_inv, uint32_t half) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > half) return;
    Fr acc = n_inv;
    if (g < half) {
        acc = Fr::one();
        Fr b = w;
        for (uint32_t e = g; e; e >>= 1) {
            if (e & 1) acc = acc * b;
            b = sqr(b);
        }
    }
    store<FrCfg>(tw + 32 * (size_t)g, from_mont(acc));
}

__global__ void k_ecntt_gather(uint8_t* __restrict__ W, const uint8_t* __restrict__ in, int log_n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >> log_n) return;
    store_affine<Fq>(W, i, load_affine<Fq>(in, ecntt_bitrev(i, log_n)));
}

// J[i] = [tw[si]] in[bitrev i] for the cn points from i0 on; lane l of the launch owns table row l
__global__ __launch_bounds__(SM_BLOCK) void k_ecntt_scale(const uint8_t* __restrict__ in,
                                                          const uint8_t* __restrict__ tw, uint32_t si,
                                                          uint8_t* __restrict__ J, uint8_t* __restrict__ tbl,
                                                          uint32_t i0, uint32_t cn, int log_n) {
    using namespace r28;
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= cn) return;
    const uint32_t i = i0 + l;
    const Affine<Fq> b = load_affine<Fq>(in, ecntt_bitrev(i, log_n));
    uint8_t* o = J + (size_t)i * 144;
    if (b.is_inf()) {
        sm::store_j28(o, J28::inf());
        return;
    }
    sm::store_j28(o, sm::g1_glv_mul<false>(b, tw, si, tbl + (size_t)l * (SM_G1_ROWS * SM_G1_ROW)));
}

namespace ecn {
using namespace r28;

MBLS_DEV J28 from_affine(const Affine<Fq>& a) {  // a not the identity: madd's identity branch
    J28 r = J28::inf();
    madd(r, unpack_shift8(a.x.v), unpack_shift8(a.y.v));
    return r;
}
MBLS_DEV void store_neg(uint8_t* p, const J28& a) {  // -a: Y negated on its canonical words
    Fq y;
    to_words(a.y, y.v);
    sm::st28(p, a.x);
    store<FqCfg>(p + 48, neg(y));
    sm::st28(p + 96, a.z);
}

}  // namespace ecn

// stage s of k: butterflies q0 .. q0 + cn - 1 (q = block * 2^(s-1) + j); twiddle w^(j 2^(k-s))
__global__ __launch_bounds__(SM_BLOCK) void k_ecntt_stage(const uint8_t* __restrict__ W,
                                                          const uint8_t* __restrict__ tw, uint8_t* __restrict__ J,
                                                          uint8_t* __restrict__ tbl, uint32_t q0, uint32_t cn,
                                                          int s, int log_n) {
    using namespace r28;
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= cn) return;
    const uint32_t q = q0 + l, half = 1u << (s - 1), j = q & (half - 1);
    const size_t ia = ((size_t)(q >> (s - 1)) << s) + j, ib = ia + half;
    uint8_t *oa = J + ia * 144, *ob = J + ib * 144;
    const Affine<Fq> b = load_affine<Fq>(W, ib);
    if (b.is_inf()) {
        const Affine<Fq> a = load_affine<Fq>(W, ia);
        const J28 r = a.is_inf() ? J28::inf() : ecn::from_affine(a);
        sm::store_j28(oa, r);
        sm::store_j28(ob, r);
        return;
    }
    J28 t = j == 0 ? ecn::from_affine(b)
                   : sm::g1_glv_mul<false>(b, tw, (size_t)j << (log_n - s), tbl + (size_t)l * (SM_G1_ROWS * SM_G1_ROW));
    const Affine<Fq> a = load_affine<Fq>(W, ia);
    if (a.is_inf()) {
        sm::store_j28(oa, t);
        ecn::store_neg(ob, t);
        return;
    }
    const F28 ax = unpack_shift8(a.x.v);
    {
        J28 u = t;
        madd(u, ax, unpack_shift8(a.y.v));
        sm::store_j28(oa, u);
    }
    const Fq ny = neg(a.y);
    madd(t, ax, unpack_shift8(ny.v));  // t - a
    ecn::store_neg(ob, t);             // a - t
}

static Fr fr_words(const uint64_t* h) {
    Fr r;
    memcpy(r.v, h, 32);
    return r;
}

static eIcicleError ecntt_call(const mbls_g1_affine_t* input, int size, NTTDir dir, const NTTConfig* cfg,
                               mbls_g1_affine_t* output) {
    if (!input || !output || !cfg) return MBLS_INVALID_POINTER;
    if (size < 1 || (size & (size - 1)) || size > (1 << ECNTT_MAX_LOG)) return MBLS_INVALID_ARGUMENT;
    int log_n = 0;
    while ((1 << log_n) < size) ++log_n;
    if (cfg->batch_size != 0 && cfg->batch_size != 1) return MBLS_INVALID_ARGUMENT;
    if (cfg->columns_batch) return MBLS_INVALID_ARGUMENT;
    if ((int)cfg->ordering != MBLS_ORDERING_NN) return MBLS_INVALID_ARGUMENT;
    if (!fr_is_montgomery_one(cfg->coset_gen.limbs)) return MBLS_INVALID_ARGUMENT;  // no cosets
    const bool inverse = dir == MBLS_NTT_INVERSE;
    uint64_t w[4], ninv[4];
    const eIcicleError dr = ntt_domain_roots(log_n, inverse, w, ninv);
    if (dr != MBLS_SUCCESS) return dr;

    const size_t n = (size_t)size, half = n / 2;
    const size_t lanes_max = inverse ? n : (half ? half : 1);
    constexpr size_t ROW = (size_t)SM_G1_ROWS * SM_G1_ROW;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *tbl, *W, *J, *tw, *dout;
    const uint8_t* din;
    S.scratch(&tbl, (lanes_max < SM_G1_CHUNK ? lanes_max : SM_G1_CHUNK) * ROW);
    S.scratch(&W, n * 96);
    S.scratch(&J, n * 144);
    S.scratch(&tw, (half + 1) * 32);
    S.in(&din, input, n * 96, cfg->are_inputs_on_device);
    S.out(&dout, output, n * 96, cfg->are_outputs_on_device);
    const eIcicleError er = S.open();
    if (er != MBLS_SUCCESS) return er;
    {
        ProfScope prof(inverse ? "ecntt.inverse" : "ecntt.forward", st);
        hipLaunchKernelGGL(k_ecntt_twiddles, dim3((unsigned)(half / 256 + 1)), dim3(256), 0, st, tw, fr_words(w),
                           fr_words(ninv), (uint32_t)half);
        MBLS_TRY(hipGetLastError());
        if (inverse) {
            for (size_t i0 = 0; i0 < n; i0 += SM_G1_CHUNK) {  // stream order serialises the chunks on the table
                const uint32_t cn = (uint32_t)(n - i0 < SM_G1_CHUNK ? n - i0 : SM_G1_CHUNK);
                hipLaunchKernelGGL(k_ecntt_scale, dim3((cn + SM_BLOCK - 1) / SM_BLOCK), dim3(SM_BLOCK), 0, st, din, tw,
                                   (uint32_t)half, J, tbl, (uint32_t)i0, cn, log_n);
                MBLS_TRY(hipGetLastError());
            }
            const eIcicleError ne = g1_jac_to_affine_device(J, log_n ? W : dout, size, st);
            if (ne != MBLS_SUCCESS) return ne;
        } else if (log_n == 0) {
            if (dout != din) MBLS_TRY(hipMemcpyAsync(dout, din, 96, hipMemcpyDeviceToDevice, st));
        } else {
            hipLaunchKernelGGL(k_ecntt_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W, din, log_n);
            MBLS_TRY(hipGetLastError());
        }
        for (int s = 1; s <= log_n; ++s) {
            for (size_t q0 = 0; q0 < half; q0 += SM_G1_CHUNK) {
                const uint32_t cn = (uint32_t)(half - q0 < SM_G1_CHUNK ? half - q0 : SM_G1_CHUNK);
                hipLaunchKernelGGL(k_ecntt_stage, dim3((cn + SM_BLOCK - 1) / SM_BLOCK), dim3(SM_BLOCK), 0, st, W, tw, J,
                                   tbl, (uint32_t)q0, cn, s, log_n);
                MBLS_TRY(hipGetLastError());
            }
            const eIcicleError ne = g1_jac_to_affine_device(J, s == log_n ? dout : W, size, st);
            if (ne != MBLS_SUCCESS) return ne;
        }
    }
    return S.close(cfg->is_async);
}

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError mbls_g1_ecntt(const mbls_g1_affine_t* input, int size, NTTDir dir, const NTTConfig* config,
                           mbls_g1_affine_t* output) {
    return ecntt_call(input, size, dir, config, output);
}

}  // extern "C"
