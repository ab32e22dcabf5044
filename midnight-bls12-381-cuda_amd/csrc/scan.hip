// scan.hip -- Fr prefix scans along a column: the grand product z[i+1] = z[i] * num[i] / den[i] of
// the permutation and lookup arguments, and the Horner recurrence q[i-1] = a[i] + z * q[i] behind
// polynomial evaluation and division by X - z (KZG openings).  No reference counterpart: the
// reference computes both on the CPU (compute_product, eval_polynomial, kate_division).
//
// The skeleton -- geometry, operators, the tile scan and the three launches -- is mbls_scan.hpp,
// shared with the running sum of logup.hip; this file holds the product's denominators and the
// entries of the two operators with a Montgomery product per step.
//
// Scan inputs are witness-derived: no branch and no address below depends on a field value; the
// conditions are on thread, lane, tile and size only.  The denominator path keeps k_batch_inv's
// shape (vecops.hip): the fixed Fermat chain and mask selects for zeros.
#include <hip/hip_runtime.h>

#include "mbls_common.hpp"
#include "mbls_field.hpp"
#include "mbls_scan.hpp"

namespace mbls {

// ---- denominators: out[i] = num[i] * den[i]^-1 with 0^-1 = 0, k_batch_inv's two sweeps over a
// thread's contiguous chunk (`out` holds the prefix products between them) with the product by
// num folded into the second.  out may not overlap num or den: it is scratch.
static constexpr int RATIO_CHUNK = 64;
__global__ __launch_bounds__(256) void k_scan_ratio(uint8_t* __restrict__ out, const uint8_t* __restrict__ num,
                                                    const uint8_t* __restrict__ den, size_t n) {
    const size_t s = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) * RATIO_CHUNK;
    if (s >= n) return;
    const size_t e = s + RATIO_CHUNK < n ? s + RATIO_CHUNK : n;
    Fr acc = Fr::one();
    for (size_t i = s; i < e; ++i) {
        const Fr x = load<FrCfg>(den + 32 * i);
        store<FrCfg>(out + 32 * i, acc);
        acc = fr_select(zero_mask(x), acc, acc * x);
    }
    Fr inv_acc = inv_fermat(acc);
    for (size_t i = e; i-- > s;) {
        const Fr x = load<FrCfg>(den + 32 * i);
        const uint32_t z = zero_mask(x);
        const Fr xi = fr_select(z, Fr::zero(), inv_acc * load<FrCfg>(out + 32 * i));
        store<FrCfg>(out + 32 * i, load<FrCfg>(num + 32 * i) * xi);
        inv_acc = fr_select(z, inv_acc, inv_acc * x);
    }
}

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError mbls_fr_prefix_product(const mbls_fr_t* num, const mbls_fr_t* den, size_t size, const mbls_fr_t* init,
                                    bool inclusive, const VecOpsConfig* config, mbls_fr_t* output, mbls_fr_t* total) {
    if (!num || !config || !output) return MBLS_INVALID_POINTER;
    ScanCall c;
    eIcicleError er = scan_call(size, config, &c);
    if (er != MBLS_SUCCESS) return er;
    hipStream_t st = static_cast<hipStream_t>(config->stream);
    const size_t bytes = 32 * c.size * c.batch, per_member = 32 * (size_t)c.batch;
    const size_t agg_bytes = align_up(per_member * c.g.groups);

    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *scratch, *dout, *dtotal = nullptr;
    const uint8_t *dnum, *dden = nullptr, *dinit = nullptr;
    // one block: the span aggregates, the values entering the spans, then num / den if den is given
    S.scratch(&scratch, 2 * agg_bytes + (den ? bytes : 0));
    S.in(&dnum, num, bytes, config->is_a_on_device);
    if (den) S.in(&dden, den, bytes, config->is_a_on_device);
    if (init) S.in(&dinit, init, per_member, config->is_b_on_device);
    S.out(&dout, output, bytes, config->is_result_on_device);
    if (total) S.out(&dtotal, total, per_member, config->is_result_on_device);
    er = S.open();
    if (er != MBLS_SUCCESS) return er;
    uint8_t *agg = scratch, *carry = scratch + agg_bytes;
    if (den) {
        uint8_t* ratio = scratch + 2 * agg_bytes;
        const size_t n = c.size * c.batch, threads = (n + RATIO_CHUNK - 1) / RATIO_CHUNK;
        hipLaunchKernelGGL(k_scan_ratio, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, ratio, dnum, dden, n);
        dnum = ratio;
    }
    er = inclusive ? scan_launch<ScanMul, true>(c, dout, dnum, nullptr, dinit, dtotal, agg, carry, st)
                   : scan_launch<ScanMul, false>(c, dout, dnum, nullptr, dinit, dtotal, agg, carry, st);
    if (er != MBLS_SUCCESS) return er;
    return S.close(config->is_async);
}

eIcicleError mbls_fr_poly_divide_linear(const mbls_fr_t* coeffs, size_t size, const mbls_fr_t* z, const VecOpsConfig* config,
                                        mbls_fr_t* quotient, mbls_fr_t* eval) {
    if (!coeffs || !z || !config || (!quotient && !eval)) return MBLS_INVALID_POINTER;
    ScanCall c;
    eIcicleError er = scan_call(size, config, &c);
    if (er != MBLS_SUCCESS) return er;
    hipStream_t st = static_cast<hipStream_t>(config->stream);
    const size_t bytes = 32 * c.size * c.batch, per_member = 32 * (size_t)c.batch;
    const size_t agg_bytes = align_up(per_member * c.g.groups);

    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *scratch, *dq = nullptr, *deval = nullptr;
    const uint8_t *da, *dz;
    S.scratch(&scratch, 2 * agg_bytes);
    S.in(&da, coeffs, bytes, config->is_a_on_device);
    S.in(&dz, z, per_member, config->is_b_on_device);
    if (quotient) S.out(&dq, quotient, bytes, config->is_result_on_device);
    if (eval) S.out(&deval, eval, per_member, config->is_result_on_device);
    er = S.open();
    if (er != MBLS_SUCCESS) return er;
    er = scan_launch<ScanHorner, false>(c, dq, da, dz, nullptr, deval, scratch, scratch + agg_bytes, st);
    if (er != MBLS_SUCCESS) return er;
    return S.close(config->is_async);
}

eIcicleError mbls_fr_scan_geometry(size_t size, int32_t* out) {
    if (!out) return MBLS_INVALID_POINTER;
    if (size == 0 || size > SCAN_MAX_ELEMS) return MBLS_INVALID_ARGUMENT;
    const ScanGeom g = scan_geom(size);
    out[0] = SCAN_K;
    out[1] = SCAN_TILE;
    out[2] = (int32_t)g.groups;
    out[3] = (int32_t)g.span;
    return MBLS_SUCCESS;
}

}  // extern "C"
