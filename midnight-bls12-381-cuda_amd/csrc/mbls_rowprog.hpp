// mbls_rowprog.hpp -- what the two row-program evaluators share (expr.hip, the stack form; graph.hip,
// the three-address form): a caller-supplied straight-line program run once per row over columns
// read at rotated rows.  The row limit, the rotation reduction, the word-major LDS slot file of the
// kernels, and the host path of the two eval entries around an evaluator's own parts.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "mbls_common.hpp"
#include "mbls_field.hpp"

namespace mbls {

// rows, and rows per unit of rotation: a kernel forms i + off < 2 size <= 2^27 in 32 bits
static constexpr size_t ROWPROG_MAX_ROWS = (size_t)1 << 26;

// (rot * rot_stride) mod size in [0, size).  |rot * rot_stride| < 2^31 * 2^26: 64 bits hold it
static inline uint32_t rowprog_offset(int32_t rot, size_t rot_stride, size_t size) {
    const int64_t m = (int64_t)size, t = (int64_t)rot * (int64_t)rot_stride % m;
    return (uint32_t)(t < 0 ? t + m : t);
}

// The slot file of a workgroup of THREADS lanes: word w of slot s of lane t at
// ((s * 8 + w) * THREADS + t) * 4, so a wave's access to one word is 64 consecutive dwords.  A lane
// only ever touches its own words: no barrier
template <int THREADS>
MBLS_DEV void slot_put(uint32_t* sh, uint32_t slot, const Fr& v) {
#pragma unroll
    for (int w = 0; w < 8; ++w) sh[(slot * 8 + w) * THREADS + threadIdx.x] = v.v[w];
}
template <int THREADS>
MBLS_DEV Fr slot_get(const uint32_t* sh, uint32_t slot) {
    Fr r;
#pragma unroll
    for (int w = 0; w < 8; ++w) r.v[w] = sh[(slot * 8 + w) * THREADS + threadIdx.x];
    return r;
}

// the device addresses and the geometry an evaluator resolves its ops against
struct RowProgAddr {
    const uint8_t* const* columns;  // column k
    const uint8_t* constants;       // constant k at 32 k
    uint8_t* output;                // output member k at col_bytes * k
    size_t col_bytes, size, rot_stride;
};

// The eval entry of an evaluator Ev, which brings
//   Ev::Src, Ev::Op            the caller's op and the resolved op the kernel reads
//   Ev::THREADS, Ev::MAX_GRID  rows per tile, the workgroups beyond which a launch strides
//   Ev::MAX_COLUMNS
//   Ev::kernel                 (const Op*, n_ops, size, tiles)
//   check(...)                 the program rules; it keeps what lds() and resolve() need
//   lds()                      the dynamic LDS bytes of a workgroup
//   resolve(k, op, addr)       op k as the kernel reads it; called for k = 0, 1, .. in order
// Every refusal comes before the first HIP call.
template <class Ev>
eIcicleError rowprog_eval(const mbls_fr_t* const* columns, int n_columns, size_t size, size_t rot_stride,
                          const mbls_fr_t* constants, int n_constants, const typename Ev::Src* program, int n_ops,
                          int n_outputs, const VecOpsConfig* config, mbls_fr_t* output) {
    using Op = typename Ev::Op;
    if (!columns || !program || !config || !output || (!constants && n_constants > 0)) return MBLS_INVALID_POINTER;
    if (size == 0 || size > ROWPROG_MAX_ROWS || rot_stride == 0 || rot_stride > ROWPROG_MAX_ROWS)
        return MBLS_INVALID_ARGUMENT;
    Ev ev;
    eIcicleError er = ev.check(program, n_ops, n_columns, n_constants, n_outputs);
    if (er != MBLS_SUCCESS) return er;
    er = check_table(columns, n_columns, Ev::MAX_COLUMNS);
    if (er != MBLS_SUCCESS) return er;
    hipStream_t st = static_cast<hipStream_t>(config->stream);
    const size_t col_bytes = 32 * size;
    // the thread's own buffers, reused by its next call
    static thread_local std::vector<const uint8_t*> dcols;
    static thread_local std::vector<Op> resolved;
    dcols.resize((size_t)n_columns);

    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *dprog, *dout;
    const uint8_t* dconst = nullptr;
    S.scratch(&dprog, sizeof(Op) * (size_t)n_ops);
    S.in_table(dcols.data(), columns, n_columns, col_bytes, config->is_a_on_device);
    if (n_constants > 0) S.in(&dconst, constants, 32 * (size_t)n_constants, config->is_b_on_device);
    S.out(&dout, output, col_bytes * (size_t)n_outputs, config->is_result_on_device);
    er = S.open();
    if (er != MBLS_SUCCESS) return er;

    // the resolved program; the copy leaves pageable memory before hipMemcpyAsync returns, as the
    // staged operands do
    const RowProgAddr addr = {dcols.data(), dconst, dout, col_bytes, size, rot_stride};
    resolved.resize((size_t)n_ops);
    for (int k = 0; k < n_ops; ++k) resolved[(size_t)k] = ev.resolve(k, program[k], addr);
    MBLS_TRY(hipMemcpyAsync(dprog, resolved.data(), sizeof(Op) * (size_t)n_ops, hipMemcpyHostToDevice, st));

    const uint32_t tiles = (uint32_t)((size + Ev::THREADS - 1) / Ev::THREADS);
    hipLaunchKernelGGL(Ev::kernel, dim3(std::min<uint32_t>(tiles, Ev::MAX_GRID)), dim3(Ev::THREADS), ev.lds(), st,
                       reinterpret_cast<const Op*>(dprog), (uint32_t)n_ops, (uint32_t)size, tiles);
    MBLS_TRY(hipGetLastError());
    return S.close(config->is_async);
}

}  // namespace mbls
