// fixed_base.hip -- fixed-base batch multiplication, output[i] = [scalars[i] mod r] base for ONE
// base (G1 and G2), and a KZG SRS from a secret (mbls_g1_srs_from_secret: [tau^i] G and
// [L_i(tau)] G, what halo2's ParamsKZG::unsafe_setup computes).  No reference counterpart.
//
// table  table[w 2^(c-1) + (d - 1)] = [d 2^(c w)] base, d = 1 .. 2^(c-1), w < W (mbls_fixed_base.hpp):
//        the W 2^(c-1) public constants d 2^(c w) mod r are written as standard scalars beside as
//        many copies of the base (k_fixed_base_consts), multiplied by the variable-base entry in
//        one launch (mbls_g*_scalar_mul: the doublings are paid here, once per base) and normalised
//        in one (projective_to_affine).  The top window's upper rows exceed r (and 2^256): on a base
//        of order r the point of the reduced constant is the same.
// mul    k_fixed_base_g1 / _g2, one lane per scalar: k mod r (load_scalar: mbls_split.hpp's
//        reduction, from_mont first for Montgomery scalars) is recoded into W signed digits, lowest
//        window first, and every non-zero digit d_w adds row (w, |d_w|) with the sign on y -- at
//        most W mixed additions and no doubling.  A Jacobian work array in the leased arena takes
//        the sums and the existing normalisation (k_jac_to_affine) writes the canonical affine
//        output.  Launches carry at most G1_CHUNK / G2_CHUNK lanes, so the work array stays bounded
//        whatever the batch size; stream order serialises the chunks on it.
// srs    the scalars are made on the device by the Fr entries (mbls_fr_powers,
//        bls12_381_batch_inv_cuda, scalar_add_vec_cuda, vec_mul_cuda) as Montgomery elements, then
//        one multiplication runs over them.  basis 1 is the barycentric form halo2 uses:
//        L_i(tau) = c w^i / (tau - w^i), c = (tau^n - 1) / n -- no EC-NTT.
//
// G1 arithmetic: the radix-2^28 lane types (mbls_fq28.hpp) inside their documented bounds.  A row
// is canonical words through unpack_shift8 (normalised, < 256 p); a negative digit negates y on
// the canonical words (p - y, still canonical: y != 0 on a point of odd order); the accumulator
// keeps J28's invariant (madd restores it, its identity branch folds the row), so store_j28
// (to_words: any value < 2^391) writes canonical words.
// With a base of order r no partial sum equals +- the next addend (tests/fixed_base_model.py states
// it for the edge scalars and random ones), so madd's doubling and cancellation branches are not
// taken; they stay in for a base outside the subgroup.
// The nested entries lease their own scratch context while this call holds one.  Such a nested
// lease never waits for a context (common.cpp: a thread that holds a lease gets a context past the
// pool's limit when none is free), so the calls cannot deadlock the pool, whatever its limit and
// however many threads are inside them.
// Not constant time: table addresses depend on the scalar's digits.
#include <hip/hip_runtime.h>
#include <string.h>

#include "mbls_common.hpp"
#include "mbls_curve.hpp"
#include "mbls_fq28.hpp"
#include "mbls_split.hpp"
#include "mbls_scalar_mul.hpp"
#include "mbls_fixed_base.hpp"

namespace mbls {

// consts[e] = d 2^(c w) mod r for e = w 2^(c-1) + d - 1 (standard form, canonical), rep[e] = the
// base.  The top window's upper rows pass 2^256 (2^11 2^252 at c = 12), so the constant is formed
// mod r, by c w modular doublings of d: exact for every row, also those no digit reaches.
template <class F>
__global__ void k_fixed_base_consts(uint8_t* __restrict__ consts, uint8_t* __restrict__ rep,
                                    const uint8_t* __restrict__ base) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (uint32_t)fb::ENTRIES) return;
    const uint32_t w = e / fb::ROWS, d = e % fb::ROWS + 1;
    Fr x = Fr::zero();
    x.v[0] = d;  // d <= 2^15 < r
    for (uint32_t b = 0; b < w * fb::C; ++b) x = dbl(x);
    store<FrCfg>(consts + 32 * (size_t)e, x);
    store_affine<F>(rep, e, load_affine<F>(base, 0));
}

template <bool MONT>
__global__ __launch_bounds__(fb::BLOCK) void k_fixed_base_g1(const uint8_t* __restrict__ table,
                                                             const uint8_t* __restrict__ scalars,
                                                             uint8_t* __restrict__ J, uint32_t n) {
    using namespace r28;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr s = load_scalar<MONT>(scalars, i);
    uint32_t carry = 0;
    J28 acc = J28::inf();
#pragma unroll 1
    for (int w = 0; w < fb::WINDOWS; ++w) {
        const int d = fb::next_digit(s.v, carry, w == fb::WINDOWS - 1);
        if (d == 0) continue;
        const uint8_t* q = table + (size_t)fb::table_index(w, d) * 96;
        const Fq qx = load<FqCfg>(q);
        Fq qy = load<FqCfg>(q + 48);
        if (qx.is_zero() && qy.is_zero()) continue;  // the identity base
        if (d < 0) qy = neg(qy);
        madd(acc, unpack_shift8(qx.v), unpack_shift8(qy.v));
    }
    sm::store_j28(J + (size_t)i * 144, acc);
}

template <bool MONT>
__global__ __launch_bounds__(fb::BLOCK) void k_fixed_base_g2(const uint8_t* __restrict__ table,
                                                             const uint8_t* __restrict__ scalars,
                                                             uint8_t* __restrict__ J, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr s = load_scalar<MONT>(scalars, i);
    uint32_t carry = 0;
    Jacobian<Fq2> acc = Jacobian<Fq2>::inf();
#pragma unroll 1
    for (int w = 0; w < fb::WINDOWS; ++w) {
        const int d = fb::next_digit(s.v, carry, w == fb::WINDOWS - 1);
        if (d == 0) continue;
        Affine<Fq2> q = load_affine<Fq2>(table, fb::table_index(w, d));
        if (q.is_inf()) continue;  // the identity base
        if (d < 0) q.y = neg(q.y);
        acc = jac_madd(acc, q);  // its identity branch takes the first row
    }
    store_jac<Fq2>(J, i, acc);
}

// a config for the nested entries: device operands, enqueue only
static VecOpsConfig nested_config(hipStream_t st) {
    VecOpsConfig c;
    memset(&c, 0, sizeof(c));
    c.stream = st;
    c.is_a_on_device = c.is_b_on_device = c.is_result_on_device = c.is_async = true;
    return c;
}

template <bool G2>
static eIcicleError normalise(const uint8_t* J, uint8_t* out, int n, hipStream_t st) {
    if (!G2) return g1_jac_to_affine_device(J, out, n, st);
    const VecOpsConfig c = nested_config(st);
    return bls12_381_g2_projective_to_affine(reinterpret_cast<const mbls_g2_projective_t*>(J), n, &c,
                                             reinterpret_cast<mbls_g2_affine_t*>(out));
}

// out[i] = [scalars[i]] base over device operands; J: the work array of min(n, CHUNK) points
template <bool G2>
static eIcicleError fixed_base_run(const uint8_t* table, const uint8_t* ds, size_t n, bool mont, uint8_t* J,
                                   uint8_t* dout, hipStream_t st) {
    using PS = PointSize<typename std::conditional<G2, Fq2, Fq>::type>;
    constexpr size_t CHUNK = G2 ? fb::G2_CHUNK : fb::G1_CHUNK;
    ProfScope prof(G2 ? "fixed_base.g2" : "fixed_base.g1", st);
    for (size_t i0 = 0; i0 < n; i0 += CHUNK) {  // stream order serialises the chunks on J
        const uint32_t cn = (uint32_t)(n - i0 < CHUNK ? n - i0 : CHUNK);
        const dim3 grid((cn + fb::BLOCK - 1) / fb::BLOCK), block(fb::BLOCK);
        const uint8_t* cs = ds + i0 * 32;
        if (G2) {
            if (mont)
                hipLaunchKernelGGL(k_fixed_base_g2<true>, grid, block, 0, st, table, cs, J, cn);
            else
                hipLaunchKernelGGL(k_fixed_base_g2<false>, grid, block, 0, st, table, cs, J, cn);
        } else {
            if (mont)
                hipLaunchKernelGGL(k_fixed_base_g1<true>, grid, block, 0, st, table, cs, J, cn);
            else
                hipLaunchKernelGGL(k_fixed_base_g1<false>, grid, block, 0, st, table, cs, J, cn);
        }
        MBLS_TRY(hipGetLastError());
        const eIcicleError er = normalise<G2>(J, dout + i0 * PS::AFF, (int)cn, st);
        if (er != MBLS_SUCCESS) return er;
    }
    return MBLS_SUCCESS;
}

template <bool G2>
static size_t work_bytes(size_t n) {
    using PS = PointSize<typename std::conditional<G2, Fq2, Fq>::type>;
    constexpr size_t CHUNK = G2 ? fb::G2_CHUNK : fb::G1_CHUNK;
    return (n < CHUNK ? n : CHUNK) * PS::JAC;
}

template <bool G2>
static eIcicleError table_call(const void* base, const VecOpsConfig* cfg, void* table) {
    if (!base || !cfg || !table) return MBLS_INVALID_POINTER;
    using F = typename std::conditional<G2, Fq2, Fq>::type;
    using PS = PointSize<F>;
    constexpr size_t E = fb::ENTRIES;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *consts, *rep, *J;
    const uint8_t* db;
    S.scratch(&consts, E * 32);
    S.scratch(&rep, E * PS::AFF);
    S.scratch(&J, E * PS::JAC);
    S.in(&db, base, PS::AFF, cfg->is_a_on_device);
    eIcicleError er = S.open();
    if (er != MBLS_SUCCESS) return er;
    {
        ProfScope prof(G2 ? "fixed_base.table_g2" : "fixed_base.table_g1", st);
        hipLaunchKernelGGL(k_fixed_base_consts<F>, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, consts, rep, db);
        MBLS_TRY(hipGetLastError());
        const VecOpsConfig c = nested_config(st);
        if (G2)
            er = mbls_g2_scalar_mul(reinterpret_cast<const mbls_g2_affine_t*>(rep), reinterpret_cast<const mbls_fr_t*>(consts),
                                    (int)E, false, &c, reinterpret_cast<mbls_g2_projective_t*>(J));
        else
            er = mbls_g1_scalar_mul(reinterpret_cast<const mbls_g1_affine_t*>(rep), reinterpret_cast<const mbls_fr_t*>(consts),
                                    (int)E, false, &c, reinterpret_cast<mbls_g1_projective_t*>(J));
        if (er != MBLS_SUCCESS) return er;
        er = normalise<G2>(J, static_cast<uint8_t*>(table), (int)E, st);
        if (er != MBLS_SUCCESS) return er;
    }
    return S.close(cfg->is_async);
}

template <bool G2>
static eIcicleError mul_call(const void* table, const void* scalars, int size, bool mont, const VecOpsConfig* cfg,
                             void* output) {
    if (!table || !scalars || !cfg || !output) return MBLS_INVALID_POINTER;
    if (size <= 0 || size > fb::MAX_BATCH) return MBLS_INVALID_ARGUMENT;
    using PS = PointSize<typename std::conditional<G2, Fq2, Fq>::type>;
    const size_t n = (size_t)size;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *J, *dout;
    const uint8_t* ds;
    S.scratch(&J, work_bytes<G2>(n));
    S.in(&ds, scalars, n * 32, cfg->is_b_on_device);
    S.out(&dout, output, n * PS::AFF, cfg->is_result_on_device);
    eIcicleError er = S.open();
    if (er != MBLS_SUCCESS) return er;
    er = fixed_base_run<G2>(static_cast<const uint8_t*>(table), ds, n, mont, J, dout, st);
    if (er != MBLS_SUCCESS) return er;
    return S.close(cfg->is_async);
}

// ---- host Fr (Montgomery, four 64-bit limbs): the few products the SRS call decides on
typedef unsigned __int128 u128;
static const uint64_t FB_R[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL,
                                 0x73eda753299d7d48ULL};
static const uint64_t FB_ONE[4] = {0x00000001fffffffeULL, 0x5884b7fa00034802ULL, 0x998c4fefecbc4ff5ULL,
                                   0x1824b159acc5056fULL};

static bool fr_geq_r(const uint64_t* t) {
    for (int i = 3; i >= 0; --i)
        if (t[i] != FB_R[i]) return t[i] > FB_R[i];
    return true;
}
static void fr_sub_r(uint64_t* t) {
    uint64_t br = 0;
    for (int i = 0; i < 4; ++i) {
        const u128 d = (u128)t[i] - FB_R[i] - br;
        t[i] = (uint64_t)d;
        br = (uint64_t)(d >> 64) & 1;
    }
}
// a b / 2^256 mod r for a, b < r (CIOS)
static void fr_mul(uint64_t* r, const uint64_t* a, const uint64_t* b) {
    uint64_t t[6] = {0};
    for (int i = 0; i < 4; ++i) {
        uint64_t c = 0;
        for (int j = 0; j < 4; ++j) {
            const u128 s = (u128)a[j] * b[i] + t[j] + c;
            t[j] = (uint64_t)s;
            c = (uint64_t)(s >> 64);
        }
        u128 s = (u128)t[4] + c;
        t[4] = (uint64_t)s;
        t[5] = (uint64_t)(s >> 64);
        const uint64_t q = t[0] * 0xfffffffeffffffffULL;  // -r^-1 mod 2^64
        s = (u128)q * FB_R[0] + t[0];
        c = (uint64_t)(s >> 64);
        for (int j = 1; j < 4; ++j) {
            s = (u128)q * FB_R[j] + t[j] + c;
            t[j - 1] = (uint64_t)s;
            c = (uint64_t)(s >> 64);
        }
        s = (u128)t[4] + c;
        t[3] = (uint64_t)s;
        t[4] = t[5] + (uint64_t)(s >> 64);
    }
    if (t[4] != 0 || fr_geq_r(t)) fr_sub_r(t);
    memcpy(r, t, 32);
}
// a - b mod r for a, b < r
static void fr_sub(uint64_t* r, const uint64_t* a, const uint64_t* b) {
    uint64_t t[4], br = 0;
    for (int i = 0; i < 4; ++i) {
        const u128 d = (u128)a[i] - b[i] - br;
        t[i] = (uint64_t)d;
        br = (uint64_t)(d >> 64) & 1;
    }
    if (br) {
        uint64_t c = 0;
        for (int i = 0; i < 4; ++i) {
            const u128 s = (u128)t[i] + FB_R[i] + c;
            t[i] = (uint64_t)s;
            c = (uint64_t)(s >> 64);
        }
    }
    memcpy(r, t, 32);
}

static eIcicleError srs_call(const mbls_g1_affine_t* table, const mbls_fr_t* tau_in, int size, int basis,
                             const VecOpsConfig* cfg, mbls_g1_affine_t* output) {
    if (!table || !tau_in || !cfg || !output) return MBLS_INVALID_POINTER;
    if (size <= 0 || size > fb::MAX_BATCH) return MBLS_INVALID_ARGUMENT;
    if (basis != 0 && basis != 1) return MBLS_INVALID_ARGUMENT;
    uint64_t tau[4], w[4], ninv[4], coef[4], zero[4] = {0, 0, 0, 0};
    {  // any 256-bit value: reduced as the scalars are
        uint32_t t[8];
        memcpy(t, tau_in->limbs, 32);
        fb::reduce(t);
        memcpy(tau, t, 32);
    }
    if (basis == 1) {
        if (size & (size - 1)) return MBLS_INVALID_ARGUMENT;
        int log_n = 0;
        while ((1 << log_n) < size) ++log_n;
        uint64_t tn[4];  // tau^n by log_n squarings
        memcpy(tn, tau, 32);
        for (int k = 0; k < log_n; ++k) fr_mul(tn, tn, tn);
        if (memcmp(tn, FB_ONE, 32) == 0) return MBLS_INVALID_ARGUMENT;  // tau is a root of X^n - 1: a pole
        const eIcicleError dr = ntt_domain_roots(log_n, false, w, ninv);
        if (dr != MBLS_SUCCESS) return dr;
        fr_sub(tn, tn, FB_ONE);
        fr_mul(coef, tn, ninv);  // (tau^n - 1) / n
    }
    const size_t n = (size_t)size;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *J, *A, *B = nullptr, *C = nullptr, *dout;
    S.scratch(&J, work_bytes<false>(n));
    S.scratch(&A, n * 32);
    if (basis == 1) {  // no pass below runs in place
        S.scratch(&B, n * 32);
        S.scratch(&C, n * 32);
    }
    S.out(&dout, output, n * 96, cfg->is_result_on_device);
    eIcicleError er = S.open();
    if (er != MBLS_SUCCESS) return er;
    {
        ProfScope prof(basis ? "fixed_base.srs_lagrange" : "fixed_base.srs_monomial", st);
        VecOpsConfig hc = nested_config(st);  // the powers' base and init come from the host
        hc.is_b_on_device = false;
        const VecOpsConfig dc = nested_config(st);
        mbls_fr_t *a = reinterpret_cast<mbls_fr_t*>(A), *b = reinterpret_cast<mbls_fr_t*>(B),
                  *c = reinterpret_cast<mbls_fr_t*>(C);
        const uint8_t* scal = basis ? B : A;
        const mbls_fr_t* tau_m = reinterpret_cast<const mbls_fr_t*>(tau);
        if (basis == 0) {
            er = mbls_fr_powers(tau_m, nullptr, n, &hc, a);  // tau^i
            if (er != MBLS_SUCCESS) return er;
        } else {
            uint64_t minus_one[4];
            fr_sub(minus_one, zero, FB_ONE);
            er = mbls_fr_powers(reinterpret_cast<const mbls_fr_t*>(w), reinterpret_cast<const mbls_fr_t*>(minus_one), n, &hc,
                                a);  // -w^i
            if (er != MBLS_SUCCESS) return er;
            er = scalar_add_vec_cuda(b, tau_m, a, size, &dc);  // tau - w^i: never zero (tau^n != 1)
            if (er != MBLS_SUCCESS) return er;
            er = bls12_381_batch_inv_cuda(c, b, size, &dc);
            if (er != MBLS_SUCCESS) return er;
            er = mbls_fr_powers(reinterpret_cast<const mbls_fr_t*>(w), reinterpret_cast<const mbls_fr_t*>(coef), n, &hc,
                                a);  // c w^i
            if (er != MBLS_SUCCESS) return er;
            er = vec_mul_cuda(b, a, c, size, &dc);  // L_i(tau)
            if (er != MBLS_SUCCESS) return er;
        }
        er = fixed_base_run<false>(reinterpret_cast<const uint8_t*>(table), scal, n, true, J, dout, st);
        if (er != MBLS_SUCCESS) return er;
    }
    return S.close(cfg->is_async);
}

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError mbls_fixed_base_plan(int group, int64_t* out) {
    if (!out) return MBLS_INVALID_POINTER;
    if (group != 1 && group != 2) return MBLS_INVALID_ARGUMENT;
    const bool g2 = group == 2;
    out[0] = fb::C;
    out[1] = fb::WINDOWS;
    out[2] = fb::ROWS;
    out[3] = fb::ENTRIES;
    out[4] = g2 ? 192 : 96;
    out[5] = fb::BLOCK;
    out[6] = g2 ? fb::G2_CHUNK : fb::G1_CHUNK;
    out[7] = g2 ? 288 : 144;
    return MBLS_SUCCESS;
}

eIcicleError mbls_fixed_base_recode(const mbls_fr_t* scalar, int32_t* digits) {
    if (!scalar || !digits) return MBLS_INVALID_POINTER;
    uint32_t k[8];
    memcpy(k, scalar->limbs, 32);
    fb::reduce(k);
    int32_t d[fb::WINDOWS];
    fb::recode(k, d);
    for (int w = 0; w < fb::WINDOWS; ++w) digits[w] = d[w];
    return MBLS_SUCCESS;
}

eIcicleError mbls_g1_fixed_base_table(const mbls_g1_affine_t* base, const VecOpsConfig* config, mbls_g1_affine_t* table) {
    return table_call<false>(base, config, table);
}
eIcicleError mbls_g2_fixed_base_table(const mbls_g2_affine_t* base, const VecOpsConfig* config, mbls_g2_affine_t* table) {
    return table_call<true>(base, config, table);
}
eIcicleError mbls_g1_fixed_base_mul(const mbls_g1_affine_t* table, const mbls_fr_t* scalars, int size,
                                    bool scalars_montgomery, const VecOpsConfig* config, mbls_g1_affine_t* output) {
    return mul_call<false>(table, scalars, size, scalars_montgomery, config, output);
}
eIcicleError mbls_g2_fixed_base_mul(const mbls_g2_affine_t* table, const mbls_fr_t* scalars, int size,
                                    bool scalars_montgomery, const VecOpsConfig* config, mbls_g2_affine_t* output) {
    return mul_call<true>(table, scalars, size, scalars_montgomery, config, output);
}
eIcicleError mbls_g1_srs_from_secret(const mbls_g1_affine_t* table, const mbls_fr_t* tau, int size, int basis,
                                     const VecOpsConfig* config, mbls_g1_affine_t* output) {
    return srs_call(table, tau, size, basis, config, output);
}

}  // extern "C"
