// tools/latbench.hip -- latency of the serial-chain primitives on ONE wave (the MSM tail's unit
// of work): a chain of N dependent operations, time / N.  Values are arbitrary field words
// (timing only).  Build: hipcc --offload-arch=gfx950 -O3 -I../midnight-bls12-381-cuda_amd/csrc latbench.hip -o latbench
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include "mbls_curve.hpp"
#include "mbls_fips.hpp"
#include "mbls_fq28.hpp"
#include "mbls_rowfield.hpp"
#include "mbls_wavepoint.hpp"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

using namespace mbls;

MBLS_DEV RFq rf_in(const uint32_t* in, int k) {
    const uint32_t j = rowdpp::lane16();
    return {j < 12 ? in[12 * k + j] : 0u};
}

template <int OP>
__global__ __launch_bounds__(64) void k_rf(uint32_t* out, const uint32_t* in, int n) {
    RFq x = rf_in(in, 0), y = rf_in(in, 1);
    for (int i = 0; i < n; ++i) {
        if constexpr (OP == 0) x = x * y;
        if constexpr (OP == 1) x = x + y;
        if constexpr (OP == 2) x = x - y;
    }
    out[threadIdx.x] = x.v;
}

template <int OP>
__global__ __launch_bounds__(64) void k_wave(uint32_t* out, const uint32_t* in, int n) {
    Jacobian<RFq> p{rf_in(in, 0), rf_in(in, 1), rf_in(in, 2)}, q{rf_in(in, 3), rf_in(in, 4), rf_in(in, 5)};
    for (int i = 0; i < n; ++i) {
        if constexpr (OP == 0) p = wave::jdbl(p);
        if constexpr (OP == 1) p = wave::jadd(p, q);
        if constexpr (OP == 2) p = jac_dbl(p);  // row mode: one point per row
        if constexpr (OP == 3) p = jac_add(p, q);
    }
    out[threadIdx.x] = p.x.v ^ p.y.v ^ p.z.v;
}

template <int OP>
__global__ __launch_bounds__(64) void k_lane(uint32_t* out, const uint32_t* in, int n) {
    Fq x = load<FqCfg>(in), y = load<FqCfg>(in + 12);
    for (int i = 0; i < n; ++i) {
        if constexpr (OP == 0) x = fips::mul(x, y);
        if constexpr (OP == 1) x = x + y;
        if constexpr (OP == 2) x = inv(x) + y;  // binary GCD inversion chain
        if constexpr (OP == 4) {                // the same on wave-uniform (SGPR, scalar-ALU) operands
#pragma unroll
            for (int k = 0; k < 12; ++k) x.v[k] = __builtin_amdgcn_readfirstlane(x.v[k]);
            Fq z;
            binv::inverse<12>(z.v, x.v, FqCfg::MOD, FqCfg::NINV);
            x = z + y;
        }
        if constexpr (OP == 3) {                // the (x, y, 1) normalisation of one point
            Jacobian<Fq> p{x, y, x + y};
            Affine<Fq> a = jac_to_affine(p);
            x = from_mont(a.x) + from_mont(a.y);
        }
    }
    store<FqCfg>(out + 12 * threadIdx.x, x);
}

// row ops vs lane-mode Fq on random canonical inputs: 64 lanes = 4 rows, each row one element
__global__ void k_check(unsigned* bad, const uint32_t* in, int iters) {
    const uint32_t j = rowdpp::lane16(), row = (threadIdx.x >> 4) + 4 * blockIdx.x;
    RFq a = {j < 12 ? in[12 * (2 * row) + j] : 0u}, b = {j < 12 ? in[12 * (2 * row + 1) + j] : 0u};
    Fq la = load<FqCfg>(in + 12 * (2 * row)), lb = load<FqCfg>(in + 12 * (2 * row + 1));
    for (int it = 0; it < iters; ++it) {
        RFq r[5] = {a + b, a - b, b - a, a * b, a + a};
        Fq l[5] = {la + lb, la - lb, lb - la, la * lb, la + la};
        for (int k = 0; k < 5; ++k) {
            const uint32_t want = j < 12 ? l[k].v[j] : 0u;
            if (r[k].v != want) atomicAdd(bad + k, 1u);
        }
        a = r[3] + r[1];
        b = r[2] - r[4];
        la = l[3] + l[1];
        lb = l[2] - l[4];
        if (it % 7 == 3) { b = a; lb = la; }  // equal operands: a - b = 0, b - a = 0
    }
}

// pieces of one binary-GCD outer step, chained: OP 0 the 30 inner steps, 1 lincomb_shift,
// 2 lincomb_mod, 3 bitlen + top33 approximations
template <int OP>
__global__ __launch_bounds__(64) void k_binv_part(uint32_t* out, const uint32_t* in, int n) {
    uint32_t a[12], b[12];
    for (int i = 0; i < 12; ++i) {
        a[i] = in[i];
        b[i] = in[12 + i];
    }
    uint64_t xa = ((uint64_t)a[1] << 32) | a[0], xb = ((uint64_t)b[1] << 32) | b[0];
    int64_t f = 12345, g = -54321;
    for (int it = 0; it < n; ++it) {
        if constexpr (OP == 0) {
            uint64_t F0 = 1, F1 = 1ull << 32;
#pragma unroll
            for (int j = 0; j < binv::K; ++j) {
                const bool odd = (xa & 1) != 0;
                const bool lt = xa < xb;
                const bool sw = odd && lt;
                const uint64_t d = lt ? xb - xa : xa - xb;
                const uint64_t G0 = sw ? F1 : F0, G1 = sw ? F0 : F1;
                xb = sw ? xa : xb;
                xa = (odd ? d : xa) >> 1;
                F0 = odd ? G0 - G1 : G0;
                F1 = G1 << 1;
            }
            xa ^= F0 + F1 + 3;
        } else if constexpr (OP == 1) {
            uint32_t r[12];
            if (binv::lincomb_shift<12>(r, a, b, f, g)) f = -f;
            for (int i = 0; i < 12; ++i) a[i] = r[i] ^ in[i];
        } else if constexpr (OP == 2) {
            uint32_t r[12];
            binv::lincomb_mod<12>(r, a, b, f, g, FqCfg::MOD, FqCfg::NINV);
            for (int i = 0; i < 12; ++i) a[i] = r[i];
        } else {
            const int nl = binv::bitlen_or<12>(a, b);
            const int nn = nl > 64 ? nl : 64;
            xa += (a[0] & 0x7fffffffu) | (binv::top33<12>(a, nn - 33) << 31);
            xb += (b[0] & 0x7fffffffu) | (binv::top33<12>(b, nn - 33) << 31);
            a[(it & 3)] ^= (uint32_t)xa;
        }
    }
    uint32_t o = (uint32_t)xa ^ (uint32_t)xb;
    for (int i = 0; i < 12; ++i) o ^= a[i];
    out[threadIdx.x] = o;
}

// lane-mode XYZZ point operations (radix 2^28) at the shape of the lane reduction levels: one chain
// per lane, 256-thread workgroups, 1024 waves (one per SIMD).  OP 0: r28::xadd, 1: r28::xdbl.
template <int OP>
__global__ __launch_bounds__(256) void k_r28(uint32_t* out, const uint32_t* in, int n) {
    r28::X28 a, q;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    for (int i = 0; i < r28::NL; ++i) {
        a.x.l[i] = (in[i] + t) & r28::MASK, a.y.l[i] = in[14 + i] & r28::MASK;
        a.zz.l[i] = in[28 + i] & r28::MASK, a.zzz.l[i] = in[42 + i] & r28::MASK;
        q.x.l[i] = in[40 + i] & r28::MASK, q.y.l[i] = in[54 + i] & r28::MASK;
        q.zz.l[i] = in[68 + i] & r28::MASK, q.zzz.l[i] = in[82 + i] & r28::MASK;
    }
    a.x.l[13] &= 0xffff, a.y.l[13] &= 0xffff, a.zz.l[13] &= 0xffff, a.zzz.l[13] &= 0xffff;
    q.x.l[13] &= 0xffff, q.y.l[13] &= 0xffff, q.zz.l[13] &= 0xffff, q.zzz.l[13] &= 0xffff;
    for (int i = 0; i < n; ++i) {
        if constexpr (OP == 0) r28::xadd(a, q.x, q.y, q.zz, q.zzz);
        if constexpr (OP == 1) r28::xdbl(a);
    }
    uint32_t o = 0;
    for (int i = 0; i < r28::NL; ++i) o ^= a.x.l[i] ^ a.y.l[i] ^ a.zz.l[i] ^ a.zzz.l[i];
    out[t] = o;
}

// ---- what an asm statement boundary on a dependent chain costs (profiles/r08/latbench.txt) ----
// The compiler pads an asm statement with one wait state (s_nop 0) when the next instruction reads
// a VGPR it wrote.  Each chain below exists in up to three forms: SPLIT, many short statements (the
// library's form through round 7); PACKED, as few statements as the chain can be written in (the
// library's form now, where it has one); PLAIN, compiler-emitted with no asm at all.  Static s_nop
// counts per leg: python tools/isa_chains.py tools/latbench.hip.
enum { SPLIT = 0, PACKED = 1, PLAIN = 2 };

// the radix-2^28 product as the library wrote it through round 7: a column's mads in statements of
// 8, 4, 2 and 1 (each writing a dummy SGPR pair), m P[0] a statement of its own
namespace r7 {
#define LB_STEP(A, B) "v_mad_u64_u32 %0, %1, " A ", " B ", %0\n\t"
#define LB_1 LB_STEP("%2", "%3")
#define LB_2 LB_1 LB_STEP("%4", "%5")
#define LB_4 LB_2 LB_STEP("%6", "%7") LB_STEP("%8", "%9")
#define LB_8 LB_4 LB_STEP("%10", "%11") LB_STEP("%12", "%13") LB_STEP("%14", "%15") LB_STEP("%16", "%17")
#define LB_OPS1(C, x, y, i, k) "v"(x[i]), C(y[k - (i)])
#define LB_OPS2(C, x, y, i, k) LB_OPS1(C, x, y, i, k), LB_OPS1(C, x, y, i + 1, k)
#define LB_OPS4(C, x, y, i, k) LB_OPS2(C, x, y, i, k), LB_OPS2(C, x, y, i + 2, k)
#define LB_OPS8(C, x, y, i, k) LB_OPS4(C, x, y, i, k), LB_OPS4(C, x, y, i + 4, k)
template <int K, int I, int HI, bool S, class X, class Y>
MBLS_DEV void col(uint64_t& acc, const X& x, const Y& y) {
    if constexpr (I <= HI) {
        constexpr int R = HI - I + 1, N = R >= 8 ? 8 : R >= 4 ? 4 : R >= 2 ? 2 : 1;
        uint64_t c;
#define LB_EMIT(n)                                                                             \
    if constexpr (N == n) {                                                                    \
        if constexpr (S) asm(LB_##n : "+v"(acc), "=&s"(c) : LB_OPS##n("s", x, y, I, K));      \
        else asm(LB_##n : "+v"(acc), "=&s"(c) : LB_OPS##n("v", x, y, I, K));                  \
    }
        LB_EMIT(8) LB_EMIT(4) LB_EMIT(2) LB_EMIT(1)
#undef LB_EMIT
        col<K, I + N, HI, S>(acc, x, y);
    }
}
template <int K>
MBLS_DEV void mul_cols(uint64_t& acc, uint32_t (&m)[r28::NL], r28::F28& r, const r28::F28& a, const r28::F28& b) {
    using namespace r28;
    if constexpr (K < 2 * NL - 1) {
        constexpr int LO = K > NL - 1 ? K - (NL - 1) : 0;
        r7::col<K, LO, (K < NL - 1 ? K : NL - 1), false>(acc, a.l, b.l);
        r7::col<K, LO, (K < NL ? K : NL) - 1, true>(acc, m, P);
        if constexpr (K < NL) {
            m[K] = ((uint32_t)acc * NINV) & MASK;
            uint64_t c;
            asm(LB_1 : "+v"(acc), "=&s"(c) : "v"(m[K]), "s"(P[0]));
        } else {
            r.l[K - NL] = (uint32_t)acc & MASK;
        }
        acc >>= 28;
        r7::mul_cols<K + 1>(acc, m, r, a, b);
    }
}
MBLS_DEV r28::F28 mul(const r28::F28& a, const r28::F28& b) {
    uint32_t m[r28::NL];
    r28::F28 r;
    uint64_t acc = 0;
    r7::mul_cols<0>(acc, m, r, a, b);
    r.l[r28::NL - 1] = (uint32_t)acc;
    return r;
}
}  // namespace r7

// the same product with every column written as C++ additions (what mbls_madchain.hpp's header says
// the compiler reassociates)
MBLS_DEV r28::F28 mul_plain(const r28::F28& a, const r28::F28& b) {
    using namespace r28;
    uint32_t m[NL];
    F28 r;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 2 * NL - 1; ++k) {
        const int lo = k > NL - 1 ? k - (NL - 1) : 0;
#pragma unroll
        for (int i = lo; i <= (k < NL - 1 ? k : NL - 1); ++i) acc += (uint64_t)a.l[i] * b.l[k - i];
#pragma unroll
        for (int i = lo; i < (k < NL ? k : NL); ++i) acc += (uint64_t)m[i] * P[k - i];
        if (k < NL) {
            m[k] = ((uint32_t)acc * NINV) & MASK;
            acc += (uint64_t)m[k] * P[0];
        } else {
            r.l[k - NL] = (uint32_t)acc & MASK;
        }
        acc >>= 28;
    }
    r.l[NL - 1] = (uint32_t)acc;
    return r;
}

template <int FORM>
__global__ __launch_bounds__(256) void k_r28mul(uint32_t* out, const uint32_t* in, int n) {
    r28::F28 x, y;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    for (int i = 0; i < r28::NL; ++i) x.l[i] = (in[i] + t) & r28::MASK, y.l[i] = in[14 + i] & r28::MASK;
    x.l[13] &= 0xffff, y.l[13] &= 0xffff;
    for (int i = 0; i < n; ++i) {
        if constexpr (FORM == SPLIT) x = r7::mul(x, y);
        if constexpr (FORM == PACKED) x = r28::mul(x, y);
        if constexpr (FORM == PLAIN) x = mul_plain(x, y);
    }
    uint32_t o = 0;
    for (int i = 0; i < r28::NL; ++i) o ^= x.l[i];
    out[t] = o;
}

// the row product with its CIOS rounds compiler-emitted: rf_mad_lo, rf_add32x2 and rf_add64_32 as
// C++ expressions (the carry-lookahead behind the rounds keeps the library's helpers).  The halves
// of a register pair cannot be named inside an asm statement, so a round -- which reads lo(t),
// hi(v), hi(w), lo(w) -- has no one-statement form.
MBLS_DEV RFq row_mul_plain(const RFq& a, const RFq& b) {
    const uint32_t p = RFq::mod_limb();
    const uint32_t a0n = rowdpp::bcast<0>(a.v) * FqCfg::NINV;
    uint64_t t = 0;
#define LB_RF_ROW(I)                                                                          \
    {                                                                                         \
        const uint32_t bi = rowdpp::bcast<I>(b.v);                                            \
        const uint32_t m = rowdpp::bcast<0>((uint32_t)t) * FqCfg::NINV + a0n * bi;            \
        const uint64_t v = (uint64_t)a.v * bi + (uint32_t)t;                                  \
        const uint64_t w = (uint64_t)m * p + ((t & 0xffffffff00000000ull) | (uint32_t)v);     \
        t = (uint64_t)(uint32_t)(v >> 32) + (uint32_t)(w >> 32) + rowdpp::from_up((uint32_t)w); \
    }
    LB_RF_ROW(0) LB_RF_ROW(1) LB_RF_ROW(2) LB_RF_ROW(3) LB_RF_ROW(4) LB_RF_ROW(5)
    LB_RF_ROW(6) LB_RF_ROW(7) LB_RF_ROW(8) LB_RF_ROW(9) LB_RF_ROW(10) LB_RF_ROW(11)
#undef LB_RF_ROW
    const uint32_t hi = (uint32_t)(t >> 32);
    return rf_reduce_once(rf_resolve((uint32_t)t, rowdpp::from_down(hi)));
}
template <int FORM>
__global__ __launch_bounds__(256) void k_rowmul(uint32_t* out, const uint32_t* in, int n) {
    RFq x = rf_in(in, 0), y = rf_in(in, 1);
    x.v ^= rowdpp::lane16() == 0 ? blockIdx.x : 0u;
    for (int i = 0; i < n; ++i) {
        if constexpr (FORM == SPLIT) x = x * y;
        if constexpr (FORM == PLAIN) x = row_mul_plain(x, y);
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = x.v;
}

// a bare chain: 16 dependent v_mad_u64_u32 per loop trip.  SPLIT one statement each, PACKED two
// statements of 8, PLAIN compiler-emitted (the multiplicand is the accumulator's own low word, which
// keeps the compiler from reassociating the sum; the dependence is the same one instruction deep)
template <int FORM>
__global__ __launch_bounds__(256) void k_madchain(uint32_t* out, const uint32_t* in, int n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t x[16], y[16];
    for (int i = 0; i < 16; ++i) x[i] = in[i] + t, y[i] = in[16 + i] | 1u;
    uint64_t acc = t;
    for (int it = 0; it < n; ++it) {
        if constexpr (FORM == SPLIT) {
#pragma unroll
            for (int i = 0; i < 16; ++i) asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(x[i]), "v"(y[i]) : "vcc");
        }
        if constexpr (FORM == PACKED) {
#define LB_M(i) "v_mad_u64_u32 %0, vcc, %[x" #i "], %[y" #i "], %0\n\t"
#define LB_O(i) [x##i] "v"(x[i]), [y##i] "v"(y[i])
            asm(LB_M(0) LB_M(1) LB_M(2) LB_M(3) LB_M(4) LB_M(5) LB_M(6) LB_M(7)
                : "+v"(acc) : LB_O(0), LB_O(1), LB_O(2), LB_O(3), LB_O(4), LB_O(5), LB_O(6), LB_O(7) : "vcc");
            asm(LB_M(8) LB_M(9) LB_M(10) LB_M(11) LB_M(12) LB_M(13) LB_M(14) LB_M(15)
                : "+v"(acc) : LB_O(8), LB_O(9), LB_O(10), LB_O(11), LB_O(12), LB_O(13), LB_O(14), LB_O(15) : "vcc");
#undef LB_O
#undef LB_M
        }
        if constexpr (FORM == PLAIN) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc = (uint64_t)(uint32_t)acc * y[i] + acc;
        }
    }
    out[t] = (uint32_t)acc ^ (uint32_t)(acc >> 32);
}

template <class K>
static void run_grid(const char* name, K kern, int blocks, int threads, uint32_t* out, const uint32_t* in, int n) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(kern, blocks, threads, 0, 0, out, in, 4);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(kern, blocks, threads, 0, 0, out, in, n);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    printf("%-28s %8.3f us/op  (%d ops, %.3f ms, %d waves)\n", name, ms * 1e3 / n, n, ms, blocks * threads / 64);
}

// one leg at one wave alone and at 1, 2 and 3 waves per SIMD (256-thread workgroups on 256 CUs):
// us per operation, min / median / max of 5 runs.  out holds LEG_MAX_BLOCKS * 256 words.
constexpr int LEG_MAX_BLOCKS = 768;
template <class K>
static void leg(const char* name, K kern, uint32_t* out, const uint32_t* in, int n) {
    const int blocks[4] = {1, 256, 512, LEG_MAX_BLOCKS}, threads[4] = {64, 256, 256, 256};
    const char* occ[4] = {"one wave", "1 wave/SIMD", "2 waves/SIMD", "3 waves/SIMD"};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int o = 0; o < 4; ++o) {
        float us[5];
        hipLaunchKernelGGL(kern, blocks[o], threads[o], 0, 0, out, in, 4);
        CK(hipDeviceSynchronize());
        for (int r = 0; r < 5; ++r) {
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(kern, blocks[o], threads[o], 0, 0, out, in, n);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            us[r] = ms * 1e3f / n;
        }
        for (int i = 1; i < 5; ++i)
            for (int j = i; j > 0 && us[j] < us[j - 1]; --j) {
                const float s = us[j];
                us[j] = us[j - 1];
                us[j - 1] = s;
            }
        printf("%-28s %-13s %8.4f %8.4f %8.4f us/op\n", name, occ[o], us[0], us[2], us[4]);
    }
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
}

template <class K>
static void run(const char* name, K kern, uint32_t* out, const uint32_t* in, int n) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(kern, 1, 64, 0, 0, out, in, 4);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(kern, 1, 64, 0, 0, out, in, n);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    printf("%-28s %8.3f us/op  (%d ops, %.3f ms)\n", name, ms * 1e3 / n, n, ms);
}

int main() {
    uint32_t *in, *out;
    CK(hipMalloc(&in, 4 * 12 * 8));
    CK(hipMalloc(&out, 4 * 12 * 64));
    uint32_t h[96];
    srand(7);
    for (int i = 0; i < 96; ++i) h[i] = (uint32_t)rand() * 2654435761u;
    for (int k = 0; k < 8; ++k) h[12 * k + 11] &= 0x0fffffff;
    CK(hipMemcpy(in, h, sizeof h, hipMemcpyHostToDevice));
    {
        const int rows = 4096;
        uint32_t* rin;
        CK(hipMalloc(&rin, 4 * 12 * 2 * rows));
        uint32_t* hr = (uint32_t*)malloc(4 * 12 * 2 * rows);
        for (int i = 0; i < 12 * 2 * rows; ++i) hr[i] = (uint32_t)rand() * 2654435761u ^ (uint32_t)rand();
        for (int e = 0; e < 2 * rows; ++e) {
            hr[12 * e + 11] %= 0x1a0111eau;  // < p
            if (e % 97 == 0) for (int k = 0; k < 12; ++k) hr[12 * e + k] = 0;  // zero operands
        }
        CK(hipMemcpy(rin, hr, 4 * 12 * 2 * rows, hipMemcpyHostToDevice));
        unsigned* bad;
        CK(hipMalloc(&bad, 32));
        CK(hipMemset(bad, 0, 32));
        hipLaunchKernelGGL(k_check, rows / 4, 64, 0, 0, bad, rin, 64);
        unsigned hb[5];
        CK(hipMemcpy(hb, bad, 20, hipMemcpyDeviceToHost));
        printf("row vs lane mismatches (add, sub, rsub, mul, dbl) over %d x 64: %u %u %u %u %u\n", rows, hb[0], hb[1],
               hb[2], hb[3], hb[4]);
        free(hr);
    }
    run("row Fq mul", k_rf<0>, out, in, 20000);
    run("row Fq add", k_rf<1>, out, in, 20000);
    run("row Fq sub", k_rf<2>, out, in, 20000);
    run("lane Fq mul (fips)", k_lane<0>, out, in, 20000);
    run("lane Fq add", k_lane<1>, out, in, 20000);
    run("lane Fq inverse (binary GCD)", k_lane<2>, out, in, 200);
    run("lane jac_to_affine + from_mont", k_lane<3>, out, in, 200);
    run("lane Fq inverse, uniform operands", k_lane<4>, out, in, 200);
    run("binv: 30 inner steps", k_binv_part<0>, out, in, 2000);
    run("binv: lincomb_shift", k_binv_part<1>, out, in, 2000);
    run("binv: lincomb_mod", k_binv_part<2>, out, in, 2000);
    run("binv: bitlen + top33 x2", k_binv_part<3>, out, in, 2000);
    run("wave jdbl", k_wave<0>, out, in, 2000);
    run("wave jadd", k_wave<1>, out, in, 2000);
    run("row jac_dbl", k_wave<2>, out, in, 2000);
    run("row jac_add", k_wave<3>, out, in, 2000);
    uint32_t* wide;
    CK(hipMalloc(&wide, 4 * 256 * LEG_MAX_BLOCKS));
    run_grid("lane r28 xadd, 1 wave/SIMD", k_r28<0>, 256, 256, wide, in, 400);
    run_grid("lane r28 xdbl, 1 wave/SIMD", k_r28<1>, 256, 256, wide, in, 400);
    run_grid("lane r28 xadd, one wave", k_r28<0>, 1, 64, wide, in, 400);
    run_grid("lane r28 xdbl, one wave", k_r28<1>, 1, 64, wide, in, 400);
    printf("asm statement boundaries: us/op, 5 runs each (min median max)\n");
    leg("r28 mul, split (round 7)", k_r28mul<SPLIT>, wide, in, 2000);
    leg("r28 mul, packed (library)", k_r28mul<PACKED>, wide, in, 2000);
    leg("r28 mul, plain C++", k_r28mul<PLAIN>, wide, in, 2000);
    leg("row mul, library", k_rowmul<SPLIT>, wide, in, 4000);
    leg("row mul, plain C++ rounds", k_rowmul<PLAIN>, wide, in, 4000);
    leg("16 mads, 16 statements", k_madchain<SPLIT>, wide, in, 20000);
    leg("16 mads, 2 statements", k_madchain<PACKED>, wide, in, 20000);
    leg("16 mads, plain C++", k_madchain<PLAIN>, wide, in, 20000);
    return 0;
}
