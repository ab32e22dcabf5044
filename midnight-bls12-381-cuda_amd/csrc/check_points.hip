// check_points.hip -- batch validation of G1 / G2 points: canonical words, curve equation,
// membership of the order-r subgroup.  (No reference counterpart: the reference has g1_is_on_curve,
// point.cuh:339, as a device helper only and no subgroup test.)  The MSM, the batch scalar
// multiplication and the EC-NTT split their scalars with phi = [lambda] / psi = [z], which hold
// only on the subgroup; this is the call that establishes it for an SRS, once, at upload.
//
// One lane per G1 point, a pair of lanes per G2 point, one wave per workgroup, no LDS, no table,
// no scratch rows.  Per point, in the order of mbls_point_status: every coordinate word string
// < p (on the RAW words, whatever the form), the all-zero identity, the conversion to Montgomery
// form if asked, y^2 == x^3 + b, then the endomorphism criterion of M. Scott, "A note on group
// membership tests for G1, G2 and GT on BLS pairing-friendly curves", with this library's
// constants (oracle/pyref.py):
//   G1: [z^2] P - P == phi(P), phi(x, y) = (beta x, y) = [z^2 - 1] on G1.  z^2 has 128 bits and
//       weight 17: 127 doublings and 16 mixed additions of the affine P on the radix-2^28 J28
//       chain, one more madd of -P, and the Jacobian (X, Y, Z) is compared with (beta x, y)
//       without an inversion: Z != 0, X == beta x Z^2, Y == y Z^3.
//   G2: psi(P) == [z] P = -[|z|] P.  |z| has 64 bits and weight 6: 63 doublings and 5 mixed
//       additions on the pair-sliced Jacobian<PFq2>, compared the same way with (psi(P).x,
//       -psi(P).y).
// A lane that fails a test leaves with its status; the chain is the only expensive part.  The
// chain's bits are the same for every lane, so a wave diverges only at those exits and in the
// additions' exceptional branches: a point of small order reaches the identity (or +-P) in the
// middle of its chain and walks madd's P == Q, P == -Q and identity-accumulator branches.  Both
// curve groups have odd order (h1 r, h2 r), so no doubling of a curve point gives Z == 0.
// Equalities are taken on canonical words only: J28 coordinates and radix-2^28 products are lazy
// (one field value, many limb forms), so both sides go through to_words first; the generic Fq /
// PFq2 operators return canonical values.
// Not constant time (nothing secret is involved).
#include <hip/hip_runtime.h>

#include "mbls_common.hpp"
#include "mbls_curve.hpp"
#include "mbls_scalar_mul.hpp"

namespace mbls {

static constexpr int CP_MAX_BATCH = 1 << 26;  // scalar_mul's bound (SM_MAX_BATCH)

// raw words < p (sub_mod_raw borrows exactly then)
MBLS_DEV bool cp_canonical(const Fq& a) {
    uint32_t t[12];
    return sub_mod_raw<FqCfg>(t, a.v) != 0;
}
MBLS_DEV Fq cp_four() { return dbl(dbl(Fq::one())); }

// word w of z^2 = 0xac45a401'0001a402'00000001'00000000 (GLV_LAM + 1)
MBLS_DEV uint32_t cp_z2_word(int w) {
    return w == 3 ? 0xac45a401u : w == 2 ? 0x0001a402u : w == 1 ? 0x00000001u : 0u;
}

template <bool MONT>
MBLS_DEV uint8_t check_g1(const uint8_t* __restrict__ points, uint32_t i) {
    using namespace r28;
    Affine<Fq> b = load_affine<Fq>(points, i);
    if (!cp_canonical(b.x) || !cp_canonical(b.y)) return MBLS_POINT_NONCANONICAL;
    if (b.is_inf()) return MBLS_POINT_IDENTITY;
    if (!MONT) {
        b.x = to_mont(b.x);
        b.y = to_mont(b.y);
    }
    if (!(sqr(b.y) == sqr(b.x) * b.x + cp_four())) return MBLS_POINT_OFF_CURVE;
    // acc = [z^2] P - P: bit 127 takes madd's identity branch, step -1 adds -P.  One dbl site and
    // one madd site; acc keeps J28's invariant (dbl and madd each restore it), the operands are
    // canonical words through unpack_shift8 (normalised, < 256 p), y negated on the words.
    const F28 px = unpack_shift8(b.x.v), py = unpack_shift8(b.y.v);
    const Fq ny = neg(b.y);
    const F28 pyn = unpack_shift8(ny.v);
    J28 acc = J28::inf();
#pragma unroll 1
    for (int bit = 127; bit >= -1; --bit) {
        const bool last = bit < 0;
        if (!last && !acc.is_inf()) acc = dbl(acc);
        if (last || ((cp_z2_word(bit >> 5) >> (bit & 31)) & 1)) madd(acc, px, last ? pyn : py);
    }
    if (acc.is_inf()) return MBLS_POINT_OFF_SUBGROUP;  // phi(P) is not the identity
    // (X, Y, Z) == (beta x, y): both sides of each equation to canonical words.  acc.z has limbs
    // < 2^29 (J28's invariant) against normalised partners, as in madd.
    const Fq bw = glv_beta();
    Fq lw, rw;
    to_words(acc.z, lw.v);
    if (lw.is_zero()) return MBLS_POINT_OFF_SUBGROUP;
    const F28 zz = sqr(acc.z);
    to_words(mul(mul(px, unpack_shift8(bw.v)), zz), lw.v);
    to_words(acc.x, rw.v);
    if (!(lw == rw)) return MBLS_POINT_OFF_SUBGROUP;
    to_words(mul(mul(py, acc.z), zz), lw.v);
    to_words(acc.y, rw.v);
    return lw == rw ? MBLS_POINT_OK : MBLS_POINT_OFF_SUBGROUP;
}

// G2, pair-sliced (mbls_pairfield.hpp): the two lanes of a pair hold c0 and c1 of every Fq2 value
// of ONE point and run the same steps, so both call this with the same i.  Every predicate is
// combined over the pair -- the canonical test here, PFq2's is_zero and == -- so a pair leaves
// together and stays whole inside the formulas' branches; PFq2's operators return canonical
// components.  Measured 24.3 ms at 2^20 points against 42.4 ms for the generic Jacobian<Fq2> with
// one lane per point (256 VGPRs + 108 AGPRs + 1072 B of scratch, one wave per SIMD).
static constexpr uint32_t CP_G2_LANES = LaneOf<Fq2>::LANES;

MBLS_DEV bool cp_pair_all(bool p) {
    const uint32_t v = p ? 1u : 0u;
    return (v & pairdpp::swap(v)) != 0;
}
template <bool MONT>
MBLS_DEV uint8_t check_g2(const uint8_t* __restrict__ points, uint32_t i) {
    Affine<PFq2> b = load_affine<PFq2>(points, i);
    if (!cp_pair_all(cp_canonical(b.x.v) && cp_canonical(b.y.v))) return MBLS_POINT_NONCANONICAL;
    if (b.is_inf()) return MBLS_POINT_IDENTITY;
    if (!MONT) {
        b.x.v = to_mont(b.x.v);
        b.y.v = to_mont(b.y.v);
    }
    if (!(sqr(b.y) == sqr(b.x) * b.x + PFq2{cp_four()})) return MBLS_POINT_OFF_CURVE;  // b = 4 + 4 u
    // acc = [|z|] P: bit 63 is the start, one jac_dbl site and one jac_madd site
    Jacobian<PFq2> acc = Jacobian<PFq2>::from_affine(b);
#pragma unroll 1
    for (int bit = 62; bit >= 0; --bit) {
        acc = jac_dbl(acc);
        if ((PSI_X >> bit) & 1) acc = jac_madd(acc, b);
    }
    if (acc.is_inf()) return MBLS_POINT_OFF_SUBGROUP;  // psi(P) is not the identity
    // psi(P) == -acc: X == psi(P).x Z^2 and Y == -psi(P).y Z^3
    const Affine<PFq2> q = psi_image(b);
    const PFq2 zz = sqr(acc.z);
    if (!(q.x * zz == acc.x)) return MBLS_POINT_OFF_SUBGROUP;
    return neg(q.y) * zz * acc.z == acc.y ? MBLS_POINT_OK : MBLS_POINT_OFF_SUBGROUP;
}

// status may be null (count only).  Lane t works on point t / LANES (G2: whole pairs, so lanes past
// n leave in pairs); the first lane of a point reports it.  Every lane of the wave reaches the
// ballot: lanes past n vote valid; lane 0 adds the wave's count with one ordinary atomic.
template <bool G2, bool MONT>
__global__ __launch_bounds__(SM_BLOCK) void k_check_points(const uint8_t* __restrict__ points,
                                                           uint8_t* __restrict__ status,
                                                           unsigned long long* __restrict__ n_invalid, uint32_t n) {
    constexpr uint32_t LANES = G2 ? CP_G2_LANES : 1;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = t / LANES;
    const bool first = t % LANES == 0;  // the lane that reports the point
    uint8_t s = MBLS_POINT_OK;
    if (i < n) {
        if constexpr (G2)
            s = check_g2<MONT>(points, i);
        else
            s = check_g1<MONT>(points, i);
        if (status && first) status[i] = s;
    }
    const unsigned long long bad = __ballot(first && s >= MBLS_POINT_NONCANONICAL);
    if (threadIdx.x == 0 && bad) atomicAdd(n_invalid, (unsigned long long)__popcll(bad));
}

template <bool G2>
static eIcicleError check_points_call(const void* points, int size, bool mont, const VecOpsConfig* cfg,
                                      uint8_t* status, uint64_t* n_invalid) {
    if (!points || !cfg || (!status && !n_invalid)) return MBLS_INVALID_ARGUMENT;
    if (size <= 0 || size > CP_MAX_BATCH) return MBLS_INVALID_ARGUMENT;
    constexpr size_t AFF = PointSize<typename std::conditional<G2, Fq2, Fq>::type>::AFF;
    const size_t n = (size_t)size;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *cnt, *dst = nullptr;
    const uint8_t* dp;
    S.scratch(&cnt, sizeof(unsigned long long));
    S.in(&dp, points, n * AFF, cfg->is_a_on_device);
    if (status) S.out(&dst, status, n, cfg->is_result_on_device);
    const eIcicleError er = S.open();
    if (er != MBLS_SUCCESS) return er;
    MBLS_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), st));
    {
        ProfScope prof(G2 ? "check_points.g2" : "check_points.g1", st);
        const uint32_t lanes = (uint32_t)n * (G2 ? CP_G2_LANES : 1);  // <= 2^27
        const dim3 grid((lanes + SM_BLOCK - 1) / SM_BLOCK), block(SM_BLOCK);
        unsigned long long* dc = reinterpret_cast<unsigned long long*>(cnt);
        if (mont)
            hipLaunchKernelGGL((k_check_points<G2, true>), grid, block, 0, st, dp, dst, dc, (uint32_t)n);
        else
            hipLaunchKernelGGL((k_check_points<G2, false>), grid, block, 0, st, dp, dst, dc, (uint32_t)n);
        MBLS_TRY(hipGetLastError());
    }
    // the count is a host output: it makes the call synchronous, as a host status does
    if (n_invalid) MBLS_TRY(hipMemcpyAsync(n_invalid, cnt, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    return S.close(cfg->is_async && !n_invalid);
}

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError mbls_g1_check_points(const mbls_g1_affine_t* points, int size, bool points_montgomery,
                                  const VecOpsConfig* config, uint8_t* status, uint64_t* n_invalid) {
    return check_points_call<false>(points, size, points_montgomery, config, status, n_invalid);
}
eIcicleError mbls_g2_check_points(const mbls_g2_affine_t* points, int size, bool points_montgomery,
                                  const VecOpsConfig* config, uint8_t* status, uint64_t* n_invalid) {
    return check_points_call<true>(points, size, points_montgomery, config, status, n_invalid);
}

}  // extern "C"
