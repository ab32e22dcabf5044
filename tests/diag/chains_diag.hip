// tests/diag/chains_diag.hip -- test probe for the packed mad chains (test infrastructure).
//
// Runs ONE radix-2^28 product of csrc/mbls_fq28.hpp -- mul, sqr, mul2 or mul4, the four users of
// mbls_madchain.hpp's packed column -- per lane on caller-chosen raw limbs and returns the raw output
// limbs, so that tests/test_gpu_chains.py can compare every limb with Python integers.  Compiled from
// the same headers the kernels use; nothing here is part of the product.
// Built by __graft_entry__.build(): hipcc -shared -fPIC ... -> tests/diag/libchains_diag.so
#include <hip/hip_runtime.h>

#include "mbls_fq28.hpp"

using namespace mbls;

static constexpr int SLOT_W = 16;          // words per operand slot (14 limbs used)
static constexpr int IN_W = 8 * SLOT_W;    // words per case: operands x0..x7
static constexpr int OUT_W = 16;           // words per case

MBLS_DEV r28::F28 f28(const uint32_t* p) {
    r28::F28 r;
#pragma unroll
    for (int i = 0; i < r28::NL; ++i) r.l[i] = p[i];
    return r;
}

// op: 0 mul(x0, x1)   1 sqr(x0)   2 mul2(x0, x1, x2, x3)   3 mul4(x0, .., x7)
__global__ void k_chains(int op, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t* x = in + (size_t)t * IN_W;
    uint32_t* o = out + (size_t)t * OUT_W;
    r28::F28 r = r28::F28::zero();
    switch (op) {
        case 0: r = r28::mul(f28(x), f28(x + SLOT_W)); break;
        case 1: r = r28::sqr(f28(x)); break;
        case 2: r = r28::mul2(f28(x), f28(x + SLOT_W), f28(x + 2 * SLOT_W), f28(x + 3 * SLOT_W)); break;
        case 3:
            r = r28::mul4(f28(x), f28(x + SLOT_W), f28(x + 2 * SLOT_W), f28(x + 3 * SLOT_W), f28(x + 4 * SLOT_W),
                          f28(x + 5 * SLOT_W), f28(x + 6 * SLOT_W), f28(x + 7 * SLOT_W));
            break;
        default: r.l[0] = 0xdeadbeefu; break;
    }
#pragma unroll
    for (int i = 0; i < r28::NL; ++i) o[i] = r.l[i];
}

extern "C" {
// n cases of IN_W input words -> n cases of OUT_W output words (host arrays); 0 on success
int chains_diag_run(int op, const uint32_t* in, uint32_t* out, int n) {
    if (n <= 0 || !in || !out) return -1;
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
        hipLaunchKernelGGL(k_chains, dim3((n + 63) / 64), dim3(64), 0, 0, op, d_in, d_out, n);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -4;
    }
    if (!rc && hipMemcpy(out, d_out, bo, hipMemcpyDeviceToHost) != hipSuccess) rc = -5;
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}
int chains_diag_in_words(void) { return IN_W; }
int chains_diag_out_words(void) { return OUT_W; }
}
