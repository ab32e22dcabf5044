// tests/diag/field_diag.hip -- test probe for the saturated 32-bit-limb field arithmetic (test
// infrastructure): the scalar Fq / Fr / Fq2 (csrc/mbls_field.hpp, mbls_fips.hpp), the row-sliced
// RFq / RFq2 (mbls_rowfield.hpp), the pair-sliced PFq2 (mbls_pairfield.hpp) and the wave-parallel
// point formulas (mbls_wavepoint.hpp).
//
// Runs ONE operation per launch on caller-chosen raw words -- operands built so that limb sums hit
// 0xffffffff, limb differences hit 0, borrows run through every limb, t == p inside the reduction:
// what random curve points produce once per 2^32 operations -- and returns the raw output words, so
// that tests/test_gpu_field.py can compare every result with Python integers.  Compiled from the
// headers the kernels use; nothing here is part of the product.
// Built by __graft_entry__.build(): hipcc -shared -fPIC ... -> tests/diag/libfield_diag.so
#include <hip/hip_runtime.h>

#include "mbls_curve.hpp"
#include "mbls_field.hpp"
#include "mbls_pairfield.hpp"
#include "mbls_rowfield.hpp"
#include "mbls_wavepoint.hpp"

using namespace mbls;

static constexpr int SLOT = 12;          // words per operand slot (an Fq; an Fr uses the low 8)
static constexpr int IN_W = 12 * SLOT;   // words per case: 12 slots (two Jacobian<Fq2>)
static constexpr int OUT_W = 384;        // words per case (wave G2: 5 blocks of 72)

// op = 100 * family + sub (tests/field_cases.py names them)
//   family 0 / 1: scalar Fq / Fr, one case per lane (sub 15, inv_quad: one case per DPP quad, lane k
//                 of the quad writes its result to words 12 k)
//   family 2:     row, one case per 16-lane row; results are written lane by lane (16 words per
//                 element, pad lanes included), except sub 18 (rf_load / rf_store)
//   family 3:     pair, one case per lane pair (c0 || c1, 24 words)
//   family 4:     wave, one case per wave

template <class C>
MBLS_DEV Fp<C> ldf(const uint32_t* x, int slot) {
    Fp<C> r;
#pragma unroll
    for (int i = 0; i < C::N; ++i) r.v[i] = x[slot * SLOT + i];
    return r;
}
template <class C>
MBLS_DEV void stf(uint32_t* o, int slot, const Fp<C>& a) {
#pragma unroll
    for (int i = 0; i < C::N; ++i) o[slot * SLOT + i] = a.v[i];
}
MBLS_DEV Fq2 ldf2(const uint32_t* x, int slot) { return {ldf<FqCfg>(x, slot), ldf<FqCfg>(x, slot + 1)}; }
MBLS_DEV void stf2(uint32_t* o, int slot, const Fq2& a) {
    stf(o, slot, a.c0);
    stf(o, slot + 1, a.c1);
}

// ------------------------------------------------------------------------------- scalar
// sub: 0 +  1 -  2 neg  3 dbl  4 operator*  5 mul_cios  6 sqr  7 fips::mul<C, false>
//      8 fips::sqr<C, false>  9 fips::mul2<C, true>  10 fips::mul2<C, false>  11 to_mont
//      12 from_mont  13 inv  14 inv_fermat  16 is_zero  17 ==
template <class C>
MBLS_DEV bool scalar_common(int sub, const uint32_t* x, uint32_t* o) {
    using F = Fp<C>;
    const F a = ldf<C>(x, 0), b = ldf<C>(x, 1);
    switch (sub) {
        case 0: stf(o, 0, a + b); return true;
        case 1: stf(o, 0, a - b); return true;
        case 2: stf(o, 0, neg(a)); return true;
        case 3: stf(o, 0, dbl(a)); return true;
        case 4: stf(o, 0, a * b); return true;
        case 5: stf(o, 0, mul_cios(a, b)); return true;
        case 6: stf(o, 0, sqr(a)); return true;
        case 7: stf(o, 0, fips::mul<C, false>(a, b)); return true;
        case 8: stf(o, 0, fips::sqr<C, false>(a)); return true;
        case 9: stf(o, 0, fips::mul2<C, true>(a, b, ldf<C>(x, 2), ldf<C>(x, 3))); return true;
        case 10: stf(o, 0, fips::mul2<C, false>(a, b, ldf<C>(x, 2), ldf<C>(x, 3))); return true;
        case 11: stf(o, 0, to_mont(a)); return true;
        case 12: stf(o, 0, from_mont(a)); return true;
        case 13: stf(o, 0, inv(a)); return true;
        case 14: stf(o, 0, inv_fermat(a)); return true;
        case 16: o[0] = a.is_zero() ? 1u : 0u; return true;
        case 17: o[0] = (a == b) ? 1u : 0u; return true;
        default: return false;
    }
}

__global__ void k_scalar_fr(int sub, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    uint32_t* o = out + (size_t)t * OUT_W;
    if (!scalar_common<FrCfg>(sub, in + (size_t)t * IN_W, o)) o[0] = 0xdeadbeefu;
}

// Fq only -- sub: 20 add_in  21 x2_in  22 x4_in  23 neg_in (raw)
//   24 add_in(x0, x1) * x2   25 x2_in(x0) * x1   26 x4_in(x0) * x1   27 neg_in(x0) * x1
//   28 sqr(add_in(add_in(x0, x1), x2))   29 add_in(add_in(x0, x1), x2) * add_in(add_in(x3, x4), x5)
//   Fq2 (a = x0, x1; b = x2, x3): 30 *  31 sqr  32 inv  33 +  34 -  35 is_zero  36 ==
//   37 mul2 as PFq2::operator* forms it: lane 0 a0 b0 + a1 neg_in(b1), lane 1 a1 b0 + a0 b1 (24 words)
//   38 Fq2 inv_quad (k_quad_fq2: lane k of the quad writes its result to words 24 k)
__global__ void k_scalar_fq(int sub, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t* x = in + (size_t)t * IN_W;
    uint32_t* o = out + (size_t)t * OUT_W;
    if (scalar_common<FqCfg>(sub, x, o)) return;
    const Fq a = ldf<FqCfg>(x, 0), b = ldf<FqCfg>(x, 1), c = ldf<FqCfg>(x, 2);
    switch (sub) {
        case 20: stf(o, 0, add_in(a, b)); break;
        case 21: stf(o, 0, x2_in(a)); break;
        case 22: stf(o, 0, x4_in(a)); break;
        case 23: stf(o, 0, neg_in(a)); break;
        case 24: stf(o, 0, add_in(a, b) * c); break;
        case 25: stf(o, 0, x2_in(a) * b); break;
        case 26: stf(o, 0, x4_in(a) * b); break;
        case 27: stf(o, 0, neg_in(a) * b); break;
        case 28: stf(o, 0, sqr(add_in(add_in(a, b), c))); break;
        case 29:
            stf(o, 0, add_in(add_in(a, b), c) * add_in(add_in(ldf<FqCfg>(x, 3), ldf<FqCfg>(x, 4)), ldf<FqCfg>(x, 5)));
            break;
        case 30: stf2(o, 0, ldf2(x, 0) * ldf2(x, 2)); break;
        case 31: stf2(o, 0, sqr(ldf2(x, 0))); break;
        case 32: stf2(o, 0, inv(ldf2(x, 0))); break;
        case 33: stf2(o, 0, ldf2(x, 0) + ldf2(x, 2)); break;
        case 34: stf2(o, 0, ldf2(x, 0) - ldf2(x, 2)); break;
        case 35: o[0] = ldf2(x, 0).is_zero() ? 1u : 0u; break;
        case 36: o[0] = (ldf2(x, 0) == ldf2(x, 2)) ? 1u : 0u; break;
        case 37: {
            const Fq b0 = c, b1 = ldf<FqCfg>(x, 3);
            stf(o, 0, fips::mul2(a, b0, b, neg_in(b1)));
            stf(o, 1, fips::mul2(b, b0, a, b1));
            break;
        }
        default: o[0] = 0xdeadbeefu; break;
    }
}

// inv_quad: the four lanes of a DPP quad hold the same input; whole quads exit together
template <class C>
__global__ void k_quad(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = t >> 2;
    if (e >= n) return;
    stf(out + (size_t)e * OUT_W, t & 3, inv_quad(ldf<C>(in + (size_t)e * IN_W, 0)));
}
__global__ void k_quad_fq2(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = t >> 2;
    if (e >= n) return;
    stf2(out + (size_t)e * OUT_W, 2 * (t & 3), inv_quad(ldf2(in + (size_t)e * IN_W, 0)));
}

// ------------------------------------------------------------------------------- row
MBLS_DEV void put_row(uint32_t* o, int elem, const RFq& a) { o[16 * elem + rowdpp::lane16()] = a.v; }
MBLS_DEV void put_row2(uint32_t* o, const RFq2& a) {
    put_row(o, 0, a.c0);
    put_row(o, 1, a.c1);
}
MBLS_DEV void put_flag(uint32_t* o, bool f) { o[rowdpp::lane16()] = f ? 1u : 0u; }

// sub: 0 +  1 -  2 neg  3 dbl  4 *  5 sqr  6 add_in  7 x2_in  8 x4_in  9 x8_in (raw)
//   10 add_in(x0, x1) * x2   11 x2_in(x0) * x1   12 x4_in(x0) * x1   13 x8_in(x0) * x1
//   14 from_mont  15 inv  16 is_zero  17 ==  18 rf_load -> rf_store (12 words)
//   19 sqr(add_in(add_in(x0, x1), x2))   20 x0 * RFq::r2() (to Montgomery form)
//   RFq2 (a = x0, x1; b = x2, x3): 30 +  31 -  32 *  33 sqr  34 inv  35 is_zero  36 ==  37 neg  38 dbl
// A launch whose n is no multiple of 4 leaves a wave with exited trailing rows.
__global__ void k_row(int sub, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = t >> 4;
    if (e >= n) return;
    const uint8_t* x = reinterpret_cast<const uint8_t*>(in + (size_t)e * IN_W);
    uint32_t* o = out + (size_t)e * OUT_W;
    const RFq a = rf_load(x, 0), b = rf_load(x, 1), c = rf_load(x, 2);
    const RFq2 a2 = RowOf<Fq2>::ld(x, 0), b2 = RowOf<Fq2>::ld(x, 2);
    switch (sub) {
        case 0: put_row(o, 0, a + b); break;
        case 1: put_row(o, 0, a - b); break;
        case 2: put_row(o, 0, neg(a)); break;
        case 3: put_row(o, 0, dbl(a)); break;
        case 4: put_row(o, 0, a * b); break;
        case 5: put_row(o, 0, sqr(a)); break;
        case 6: put_row(o, 0, add_in(a, b)); break;
        case 7: put_row(o, 0, x2_in(a)); break;
        case 8: put_row(o, 0, x4_in(a)); break;
        case 9: put_row(o, 0, x8_in(a)); break;
        case 10: put_row(o, 0, add_in(a, b) * c); break;
        case 11: put_row(o, 0, x2_in(a) * b); break;
        case 12: put_row(o, 0, x4_in(a) * b); break;
        case 13: put_row(o, 0, x8_in(a) * b); break;
        case 14: put_row(o, 0, from_mont(a)); break;
        case 15: put_row(o, 0, inv(a)); break;
        case 16: put_flag(o, a.is_zero()); break;
        case 17: put_flag(o, a == b); break;
        case 18: rf_store(reinterpret_cast<uint8_t*>(o), 0, a); break;
        case 19: put_row(o, 0, sqr(add_in(add_in(a, b), c))); break;
        case 20: put_row(o, 0, a * RFq::r2()); break;
        case 37: put_row2(o, neg(a2)); break;
        case 38: put_row2(o, dbl(a2)); break;
        case 30: put_row2(o, a2 + b2); break;
        case 31: put_row2(o, a2 - b2); break;
        case 32: put_row2(o, a2 * b2); break;
        case 33: put_row2(o, sqr(a2)); break;
        case 34: put_row2(o, inv(a2)); break;
        case 35: put_flag(o, a2.is_zero()); break;
        case 36: put_flag(o, a2 == b2); break;
        default: o[rowdpp::lane16()] = 0xdeadbeefu; break;
    }
}

// ------------------------------------------------------------------------------- pair
// sub: 0 +  1 -  2 neg  3 dbl  4 *  5 sqr  6 inv  7 is_zero  8 ==  9 one()   (a = x0, x1; b = x2, x3)
__global__ void k_pair(int sub, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = t >> 1;
    if (e >= n) return;
    const uint8_t* x = reinterpret_cast<const uint8_t*>(in + (size_t)e * IN_W);
    uint32_t* o = out + (size_t)e * OUT_W;
    uint8_t* ob = reinterpret_cast<uint8_t*>(o);
    const PFq2 a = FieldIO<PFq2>::ld(x), b = FieldIO<PFq2>::ld(x + 96);
    switch (sub) {
        case 0: FieldIO<PFq2>::st(ob, a + b); break;
        case 1: FieldIO<PFq2>::st(ob, a - b); break;
        case 2: FieldIO<PFq2>::st(ob, neg(a)); break;
        case 3: FieldIO<PFq2>::st(ob, dbl(a)); break;
        case 4: FieldIO<PFq2>::st(ob, a * b); break;
        case 5: FieldIO<PFq2>::st(ob, sqr(a)); break;
        case 6: FieldIO<PFq2>::st(ob, inv(a)); break;
        case 7: o[t & 1] = a.is_zero() ? 1u : 0u; break;
        case 8: o[t & 1] = (a == b) ? 1u : 0u; break;
        case 9: FieldIO<PFq2>::st(ob, PFq2::one()); break;
        default: o[t & 1] = 0xdeadbeefu; break;
    }
}

// ------------------------------------------------------------------------------- wave
// one point operation per wave, every row loaded with the same point(s): p = slots 0.. (x, y, z),
// q after it.  Output blocks of 3 field elements: block 0 stored from the leader row, blocks 1..3
// from rows 1..3, block 4 the scalar jac_dbl / jac_add of the same input (lane 0).
template <class F, bool ADD>
__global__ void k_wave(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
    using RF = typename RowOf<F>::type;
    constexpr int FQS = RowOf<F>::FQS;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = t >> 6;
    if (e >= n) return;
    const uint8_t* x = reinterpret_cast<const uint8_t*>(in + (size_t)e * IN_W);
    uint8_t* o = reinterpret_cast<uint8_t*>(out + (size_t)e * OUT_W);
    const Jacobian<RF> p{RowOf<F>::ld(x, 0), RowOf<F>::ld(x, FQS), RowOf<F>::ld(x, 2 * FQS)};
    Jacobian<RF> r;
    if constexpr (ADD) {
        const Jacobian<RF> q{RowOf<F>::ld(x, 3 * FQS), RowOf<F>::ld(x, 4 * FQS), RowOf<F>::ld(x, 5 * FQS)};
        r = wave::jadd(p, q);
    } else {
        r = wave::jdbl(p);
    }
    const size_t blk = (size_t)(wave::leader_row() ? 0u : wave::row()) * 3 * FQS;
    RowOf<F>::st(o, blk, r.x);
    RowOf<F>::st(o, blk + FQS, r.y);
    RowOf<F>::st(o, blk + 2 * FQS, r.z);
    if ((t & 63) == 0) {
        const Jacobian<F> ps = load_jac<F>(x, 0);
        Jacobian<F> rs;
        if constexpr (ADD)
            rs = jac_add(ps, load_jac<F>(x, 1));
        else
            rs = jac_dbl(ps);
        store_jac<F>(o + (size_t)4 * 3 * FQS * 48, 0, rs);
    }
}

extern "C" {
// n cases of IN_W input words -> n cases of OUT_W output words (host arrays); 0 on success
int field_diag_run(int op, const uint32_t* in, uint32_t* out, int n) {
    if (n <= 0 || n > (1 << 16) || !in || !out) return -1;
    const int fam = op / 100, sub = op % 100;
    if (fam < 0 || fam > 4) return -1;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    const size_t bi = (size_t)n * IN_W * 4, bo = (size_t)n * OUT_W * 4;
    if (hipMalloc(&d_in, bi) != hipSuccess) return -2;
    if (hipMalloc(&d_out, bo) != hipSuccess) {
        (void)hipFree(d_in);
        return -2;
    }
    int rc = 0;
    if (hipMemcpy(d_in, in, bi, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_out, 0, bo) != hipSuccess) rc = -3;
    if (!rc) {
        const dim3 blk(64);
        auto grid = [&](int lanes_per_case) { return dim3(((size_t)n * lanes_per_case + 63) / 64); };
        if (fam == 0 && sub == 15)
            hipLaunchKernelGGL(k_quad<FqCfg>, grid(4), blk, 0, 0, d_in, d_out, n);
        else if (fam == 0 && sub == 38)
            hipLaunchKernelGGL(k_quad_fq2, grid(4), blk, 0, 0, d_in, d_out, n);
        else if (fam == 1 && sub == 15)
            hipLaunchKernelGGL(k_quad<FrCfg>, grid(4), blk, 0, 0, d_in, d_out, n);
        else if (fam == 0)
            hipLaunchKernelGGL(k_scalar_fq, grid(1), blk, 0, 0, sub, d_in, d_out, n);
        else if (fam == 1)
            hipLaunchKernelGGL(k_scalar_fr, grid(1), blk, 0, 0, sub, d_in, d_out, n);
        else if (fam == 2)
            hipLaunchKernelGGL(k_row, grid(16), blk, 0, 0, sub, d_in, d_out, n);
        else if (fam == 3)
            hipLaunchKernelGGL(k_pair, grid(2), blk, 0, 0, sub, d_in, d_out, n);
        else if (sub == 0)
            hipLaunchKernelGGL((k_wave<Fq, false>), grid(64), blk, 0, 0, d_in, d_out, n);
        else if (sub == 1)
            hipLaunchKernelGGL((k_wave<Fq, true>), grid(64), blk, 0, 0, d_in, d_out, n);
        else if (sub == 2)
            hipLaunchKernelGGL((k_wave<Fq2, false>), grid(64), blk, 0, 0, d_in, d_out, n);
        else if (sub == 3)
            hipLaunchKernelGGL((k_wave<Fq2, true>), grid(64), blk, 0, 0, d_in, d_out, n);
        else
            rc = -1;
        if (!rc && (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)) rc = -4;
    }
    if (!rc && hipMemcpy(out, d_out, bo, hipMemcpyDeviceToHost) != hipSuccess) rc = -5;
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}
int field_diag_in_words(void) { return IN_W; }
int field_diag_out_words(void) { return OUT_W; }
}
