// tests/diag/chains_probe.hip -- one small kernel per arithmetic primitive, compiled to assembly by
// tests/test_isa_chains.py, which counts what the compiler made of the inline-asm chains: the
// v_mad_u64_u32 of the formula, and the wait states (`s_nop`) it pads asm statements with.
// Never run: the kernels only have to keep their primitive alive.
#include <hip/hip_runtime.h>
#include "mbls_fq28.hpp"
#include "mbls_fr29.hpp"
#include "mbls_rowfield.hpp"

using namespace mbls;

MBLS_DEV r28::F28 ld28(const uint32_t* in, int k) {
    r28::F28 a;
    for (int i = 0; i < r28::NL; ++i) a.l[i] = in[(k * r28::NL + i) * 64 + threadIdx.x];
    return a;
}
MBLS_DEV void st28(uint32_t* out, const r28::F28& a) {
    for (int i = 0; i < r28::NL; ++i) out[i * 64 + threadIdx.x] = a.l[i];
}

extern "C" __global__ __launch_bounds__(64) void probe_r28_mul(uint32_t* out, const uint32_t* in) {
    st28(out, r28::mul(ld28(in, 0), ld28(in, 1)));
}
extern "C" __global__ __launch_bounds__(64) void probe_r28_sqr(uint32_t* out, const uint32_t* in) {
    st28(out, r28::sqr(ld28(in, 0)));
}
extern "C" __global__ __launch_bounds__(64) void probe_r28_mul2(uint32_t* out, const uint32_t* in) {
    st28(out, r28::mul2(ld28(in, 0), ld28(in, 1), ld28(in, 2), ld28(in, 3)));
}
extern "C" __global__ __launch_bounds__(64) void probe_r28_mul4(uint32_t* out, const uint32_t* in) {
    st28(out, r28::mul4(ld28(in, 0), ld28(in, 1), ld28(in, 2), ld28(in, 3), ld28(in, 4), ld28(in, 5), ld28(in, 6),
                        ld28(in, 7)));
}
extern "C" __global__ __launch_bounds__(64) void probe_r29_mul_words(uint32_t* out, const uint32_t* in) {
    Fr x;
    r29::F29 w;
    for (int i = 0; i < 8; ++i) x.v[i] = in[i * 64 + threadIdx.x];
    for (int i = 0; i < r29::NL; ++i) w.l[i] = in[(8 + i) * 64 + threadIdx.x];
    const Fr y = r29::mul_words(x, w);
    for (int i = 0; i < 8; ++i) out[i * 64 + threadIdx.x] = y.v[i];
}
extern "C" __global__ __launch_bounds__(64) void probe_row_mul(uint32_t* out, const uint32_t* in) {
    const RFq a = {in[threadIdx.x]}, b = {in[64 + threadIdx.x]};
    out[threadIdx.x] = (a * b).v;
}
extern "C" __global__ __launch_bounds__(64) void probe_row_add(uint32_t* out, const uint32_t* in) {
    const RFq a = {in[threadIdx.x]}, b = {in[64 + threadIdx.x]};
    out[threadIdx.x] = (a + b).v;
}
extern "C" __global__ __launch_bounds__(64) void probe_row_sub(uint32_t* out, const uint32_t* in) {
    const RFq a = {in[threadIdx.x]}, b = {in[64 + threadIdx.x]};
    out[threadIdx.x] = (a - b).v;
}
