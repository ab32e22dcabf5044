// logup.hip -- the log-derivative lookup argument ("mv-lookup", LogUp) of halo2 forks on the device:
// the multiplicity column m, the Fr running sum, and the fused sum phi of the lookup's terms.  No
// reference counterpart: the reference tree uses the classic lookup, on the CPU.
//
// Multiplicities (design (a) of DESIGN.md 5.13): the TABLE alone is sorted (sort.hip's stable sort,
// all members in one array), then every input cell binary-searches its member's sorted keys and
// adds one to a 64-bit count at the credited row of the run it lands in:
//   sort_launch      the sorted permutation of the table rows (global row numbers);
//   k_logup_keys     the sorted standard-form keys, contiguous (they take the key planes' place);
//   k_logup_count    one search per cell, a fixed number of halvings with a clamped index and no
//                    early exit; equal targets are merged within the wave by ballots, and a wave
//                    whose rounds all hit one row carries the count in a register, so a column of
//                    one padding value costs one atomic per wave, not one per cell;
//   k_logup_emit     the counts as Fr elements (one product by R^2 when Montgomery).
// The stable sort puts equal table values in ascending row order, so the lowest row of a value is
// the first of its run (the lower bound) and the highest is the last (the upper bound, less one).
// Integer adds commute: the counts do not depend on arrival order.  A cell whose value the table
// lacks adds to a count of its member kept behind the rows.
//
// Terms and sum.  Per row the K + 1 inverses are never formed one by one: the row folds its
// denominators d into a fraction N / D = sum 1 / d, two products per denominator,
//   (N, D) -> (N d + D, D d);     the table's:  (N, D) -> (N d - m D, D d),
// a zero d leaves (N, D) alone (0^-1 = 0, by mask select), so D is a product of non-zero values.
// The D of a thread's rows then share one Fermat chain (k_batch_inv's two sweeps), and the
// additive scan (mbls_scan.hpp) runs over the terms N / D.
//
// Timing: k_logup_count is NOT constant time (bins, the search path, merged lanes).  The terms and
// the scans have no branch and no address that depends on a field value.
#include <hip/hip_runtime.h>

#include "mbls_common.hpp"
#include "mbls_field.hpp"
#include "mbls_scan.hpp"
#include "mbls_sort.hpp"

namespace mbls {

static constexpr int LOGUP_MAX_INPUTS = 64;
static constexpr int LOGUP_ROUNDS = 16;  // rows a lane searches for, one after another
static constexpr int LOGUP_MAX_CHUNK = 64, LOGUP_MIN_CHUNK = 8;

// the input columns, device pointers, by value in the kernel arguments
struct LogupCols {
    const uint8_t* p[LOGUP_MAX_INPUTS];
};

// ---- keys[i] = the standard-form key of the i-th smallest table row of all members
__global__ __launch_bounds__(SORT_THREADS) void k_logup_keys(uint8_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                             const uint8_t* __restrict__ table, uint32_t n, bool mont) {
    const uint32_t i = blockIdx.x * SORT_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t g = idx[i];
    if (g >= n) g = i;  // never, for a permutation
    store<FrCfg>(keys + 32 * (size_t)i, sort_key(load<FrCfg>(table + 32 * (size_t)g), mont));
}

// ---- counts[g] += the cells of column blockIdx.y whose value is credited to table row g (a global
// row number); counts[n + k] += the cells of member k whose value the table lacks.  A wave walks
// LOGUP_ROUNDS rounds of 64 consecutive rows.  steps: halvings that empty an interval of `size`;
// bits: the width of n + batch - 1.
__global__ __launch_bounds__(SORT_THREADS) void k_logup_count(unsigned long long* counts, LogupCols cols,
                                                              const uint8_t* __restrict__ keys,
                                                              const uint32_t* __restrict__ idx, uint32_t size, uint32_t n,
                                                              bool mont, bool credit_last, int steps, int bits) {
    const uint32_t lane = threadIdx.x & (SORT_WAVE - 1), wave = threadIdx.x / SORT_WAVE;
    const uint8_t* col = cols.p[blockIdx.y];
    const uint32_t first = (blockIdx.x * SORT_WAVES + wave) * (uint32_t)(SORT_WAVE * LOGUP_ROUNDS);  // < 2^27
    uint32_t pend_t = 0xffffffffu;  // the row the wave's earlier rounds all hit, and how often: the
    unsigned long long pend_c = 0;  // same in every lane
    for (int r = 0; r < LOGUP_ROUNDS; ++r) {
        const uint32_t base = first + (uint32_t)r * SORT_WAVE;
        if (base >= n) break;  // the same in every lane
        const bool valid = n - base > lane;
        const uint32_t g = valid ? base + lane : n - 1;
        const uint32_t k = g / size;
        const Fr a = sort_key(load<FrCfg>(col + 32 * (size_t)g), mont);
        const uint8_t* tab = keys + 32 * (size_t)k * size;
        // first: the first key not below a; last: the first key above a
        uint32_t lo = 0, hi = size;
        for (int s = 0; s < steps; ++s) {
            const uint32_t mid = lo + (hi - lo) / 2;
            const Fr kv = load<FrCfg>(tab + 32 * (size_t)(mid < size ? mid : size - 1));
            const bool right = credit_last ? !key_less(a, kv) : key_less(kv, a);
            const bool open = lo < hi;
            lo = open && right ? mid + 1 : lo;
            hi = open && !right ? mid : hi;
        }
        uint32_t pos = credit_last ? lo - 1 : lo;  // lo == 0, last: wraps and fails the bound
        const bool inside = pos < size;
        pos = inside ? pos : 0;
        const bool found = inside && load<FrCfg>(tab + 32 * (size_t)pos) == a;
        uint32_t target = idx[(size_t)k * size + pos];
        if (!found || target >= n) target = n + k;
        const uint64_t all = __ballot(valid), peers = match_bits(target, valid, bits);
        // lane 0 is valid in every round that runs; one target in the whole wave?
        const bool uniform = __all(!valid || peers == all);
        const uint32_t t0 = __shfl(target, 0, SORT_WAVE);
        if (uniform) {
            if (t0 != pend_t) {
                if (lane == 0 && pend_c) atomicAdd(&counts[pend_t], pend_c);
                pend_t = t0;
                pend_c = 0;
            }
            pend_c += (unsigned long long)__popcll(all);
        } else if (valid && (peers & ((1ull << lane) - 1)) == 0) {
            atomicAdd(&counts[target], (unsigned long long)__popcll(peers));
        }
    }
    if (lane == 0 && pend_c) atomicAdd(&counts[pend_t], pend_c);
}

// ---- m[g] = counts[g] as a field element
__global__ __launch_bounds__(SORT_THREADS) void k_logup_emit(uint8_t* __restrict__ m,
                                                             const unsigned long long* __restrict__ counts, uint32_t n,
                                                             bool mont) {
    const uint32_t g = blockIdx.x * SORT_THREADS + threadIdx.x;
    if (g >= n) return;
    const unsigned long long c = counts[g];
    Fr x = Fr::zero();
    x.v[0] = (uint32_t)c;
    x.v[1] = (uint32_t)(c >> 32);
    store<FrCfg>(m + 32 * (size_t)g, mont ? to_mont(x) : x);
}

// ---- terms.  Thread t of a workgroup owns the rows blockIdx.x * 256 * chunk + j * 256 + t, j < chunk
// (consecutive lanes, consecutive rows).  Sweep one reads the K + 2 operands of a row once, leaves
// N in num[], D in den[] and the product of the thread's earlier D in term[]; sweep two turns
// term[] into N / D.  den may be the multiplicity column itself: a row is read and then written by
// the same thread.  num, den, term: n elements each, term and num distinct from every operand.
__global__ __launch_bounds__(256) void k_logup_terms(uint8_t* __restrict__ term, uint8_t* __restrict__ num, uint8_t* den,
                                                     LogupCols cols, int n_inputs, const uint8_t* __restrict__ table,
                                                     const uint8_t* mult, const uint8_t* __restrict__ beta, uint32_t size,
                                                     uint32_t n, int chunk) {
    const size_t first = (size_t)blockIdx.x * 256 * (size_t)chunk + threadIdx.x;
    Fr acc = Fr::one();
    for (int j = 0; j < chunk; ++j) {
        const size_t g = first + (size_t)j * 256;
        if (g >= n) break;
        const Fr b = load<FrCfg>(beta + 32 * (g / size));
        Fr N = Fr::zero(), D = Fr::one();
        for (int c = 0; c < n_inputs; ++c) {
            const Fr d = load<FrCfg>(cols.p[c] + 32 * g) + b;
            const uint32_t z = zero_mask(d);
            N = fr_select(z, N, N * d + D);
            D = fr_select(z, D, D * d);
        }
        const Fr d = load<FrCfg>(table + 32 * g) + b;
        const uint32_t z = zero_mask(d);
        N = fr_select(z, N, N * d - load<FrCfg>(mult + 32 * g) * D);
        D = fr_select(z, D, D * d);
        store<FrCfg>(term + 32 * g, acc);
        store<FrCfg>(num + 32 * g, N);
        store<FrCfg>(den + 32 * g, D);
        acc = acc * D;
    }
    Fr inv_acc = inv_fermat(acc);
    for (int j = chunk; j-- > 0;) {
        const size_t g = first + (size_t)j * 256;
        if (g >= n) continue;
        const Fr Dinv = inv_acc * load<FrCfg>(term + 32 * g);
        store<FrCfg>(term + 32 * g, load<FrCfg>(num + 32 * g) * Dinv);
        inv_acc = inv_acc * load<FrCfg>(den + 32 * g);
    }
}

static int bit_width(size_t x) {
    int b = 0;
    for (; x; x >>= 1) ++b;
    return b;
}

// rows per thread of k_logup_terms: a power of two that leaves at least one wave per SIMD
// (256 CUs x 4) where the size allows, so the Fermat chain is shared as widely as the machine stays full
static int logup_chunk(size_t n) {
    int chunk = LOGUP_MIN_CHUNK;
    while (chunk < LOGUP_MAX_CHUNK && n / ((size_t)2 * chunk) >= (size_t)1024 * 64) chunk *= 2;
    return chunk;
}

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError mbls_fr_lookup_multiplicities(const mbls_fr_t* const* inputs, int n_inputs, const mbls_fr_t* table, size_t size,
                                           bool montgomery, bool credit_last, const VecOpsConfig* config,
                                           mbls_fr_t* multiplicities, uint64_t* n_missing) {
    if (!inputs || !table || !config || !multiplicities) return MBLS_INVALID_POINTER;
    SortCall c;
    eIcicleError er = sort_call(size, config, &c);
    if (er != MBLS_SUCCESS) return er;
    er = check_table(inputs, n_inputs, LOGUP_MAX_INPUTS);
    if (er != MBLS_SUCCESS) return er;
    hipStream_t st = static_cast<hipStream_t>(config->stream);
    const size_t n = c.size * c.batch, col_bytes = 32 * n;
    const SortGeom g = sort_geom(n);
    const SortLayout L = sort_layout(n, false, c.batch);
    const size_t counts_at = L.bytes;

    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *scratch, *dm;
    const uint8_t* dtab;
    LogupCols cols{};
    // the sort's, then the counts (rows, then the members' missing cells)
    S.scratch(&scratch, counts_at + align_up(8 * (n + c.batch)));
    S.in(&dtab, table, col_bytes, config->is_a_on_device);
    S.in_table(cols.p, inputs, n_inputs, col_bytes, config->is_a_on_device);
    S.out(&dm, multiplicities, col_bytes, config->is_result_on_device);
    er = S.open();
    if (er != MBLS_SUCCESS) return er;
    const uint32_t* idx;
    er = sort_launch(g, c.size, scratch, L, dtab, nullptr, g.n, montgomery, st, &idx);
    if (er != MBLS_SUCCESS) return er;
    // the planes are done with: the sorted keys take their place
    uint8_t* keys = scratch + L.planes;
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(scratch + counts_at);
    const dim3 block(SORT_THREADS), per_row(sort_blocks(n));
    const size_t per_block = (size_t)SORT_THREADS * LOGUP_ROUNDS;
    MBLS_TRY(hipMemsetAsync(counts, 0, 8 * (n + c.batch), st));
    hipLaunchKernelGGL(k_logup_keys, per_row, block, 0, st, keys, idx, dtab, g.n, montgomery);
    hipLaunchKernelGGL(k_logup_count, dim3((unsigned)((n + per_block - 1) / per_block), (unsigned)n_inputs), block, 0, st,
                       counts, cols, keys, idx, (uint32_t)c.size, g.n, montgomery, credit_last, bit_width(c.size),
                       bit_width(n + c.batch - 1));
    hipLaunchKernelGGL(k_logup_emit, per_row, block, 0, st, dm, counts, g.n, montgomery);
    MBLS_TRY(hipGetLastError());
    if (n_missing) MBLS_TRY(hipMemcpyAsync(n_missing, counts + n, 8 * c.batch, hipMemcpyDeviceToHost, st));
    return S.close(config->is_async && !n_missing);
}

eIcicleError mbls_fr_prefix_sum(const mbls_fr_t* input, size_t size, const mbls_fr_t* init, bool inclusive,
                                const VecOpsConfig* config, mbls_fr_t* output, mbls_fr_t* total) {
    if (!input || !config || !output) return MBLS_INVALID_POINTER;
    ScanCall c;
    eIcicleError er = scan_call(size, config, &c);
    if (er != MBLS_SUCCESS) return er;
    hipStream_t st = static_cast<hipStream_t>(config->stream);
    const size_t bytes = 32 * c.size * c.batch, per_member = 32 * (size_t)c.batch;
    const size_t agg_bytes = align_up(per_member * c.g.groups);

    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *scratch, *dout, *dtotal = nullptr;
    const uint8_t *din, *dinit = nullptr;
    // the span aggregates, then the values entering the spans
    S.scratch(&scratch, 2 * agg_bytes);
    S.in(&din, input, bytes, config->is_a_on_device);
    if (init) S.in(&dinit, init, per_member, config->is_b_on_device);
    S.out(&dout, output, bytes, config->is_result_on_device);
    if (total) S.out(&dtotal, total, per_member, config->is_result_on_device);
    er = S.open();
    if (er != MBLS_SUCCESS) return er;
    er = inclusive ? scan_launch<ScanAdd, true>(c, dout, din, nullptr, dinit, dtotal, scratch, scratch + agg_bytes, st)
                   : scan_launch<ScanAdd, false>(c, dout, din, nullptr, dinit, dtotal, scratch, scratch + agg_bytes, st);
    if (er != MBLS_SUCCESS) return er;
    return S.close(config->is_async);
}

eIcicleError mbls_fr_logup_sum(const mbls_fr_t* const* inputs, int n_inputs, const mbls_fr_t* table,
                               const mbls_fr_t* multiplicities, size_t size, const mbls_fr_t* beta, const mbls_fr_t* init,
                               const VecOpsConfig* config, mbls_fr_t* output, mbls_fr_t* total) {
    if (!inputs || !table || !multiplicities || !beta || !config || !output) return MBLS_INVALID_POINTER;
    ScanCall c;
    eIcicleError er = scan_call(size, config, &c);
    if (er != MBLS_SUCCESS) return er;
    er = check_table(inputs, n_inputs, LOGUP_MAX_INPUTS);
    if (er != MBLS_SUCCESS) return er;
    hipStream_t st = static_cast<hipStream_t>(config->stream);
    const size_t n = c.size * c.batch, bytes = 32 * n, stride = align_up(bytes), per_member = 32 * (size_t)c.batch;
    const size_t agg_bytes = align_up(per_member * c.g.groups);

    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *scratch, *dout, *dtotal = nullptr;
    const uint8_t *dtab, *dmult, *dbeta, *dinit = nullptr;
    LogupCols cols{};
    // the span aggregates, the values entering the spans, the terms, then the numerators (the
    // denominators live in the output)
    S.scratch(&scratch, 2 * agg_bytes + 2 * stride);
    S.in(&dtab, table, bytes, config->is_a_on_device);
    S.in(&dmult, multiplicities, bytes, config->is_a_on_device);
    S.in_table(cols.p, inputs, n_inputs, bytes, config->is_a_on_device);
    S.in(&dbeta, beta, per_member, config->is_b_on_device);
    if (init) S.in(&dinit, init, per_member, config->is_b_on_device);
    S.out(&dout, output, bytes, config->is_result_on_device);
    if (total) S.out(&dtotal, total, per_member, config->is_result_on_device);
    er = S.open();
    if (er != MBLS_SUCCESS) return er;
    uint8_t *agg = scratch, *carry = scratch + agg_bytes, *term = scratch + 2 * agg_bytes, *num = term + stride;
    const int chunk = logup_chunk(n);
    const size_t per_block = (size_t)256 * chunk;
    hipLaunchKernelGGL(k_logup_terms, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), 0, st, term, num, dout,
                       cols, n_inputs, dtab, dmult, dbeta, (uint32_t)c.size, (uint32_t)n, chunk);
    er = scan_launch<ScanAdd, false>(c, dout, term, nullptr, dinit, dtotal, agg, carry, st);
    if (er != MBLS_SUCCESS) return er;
    return S.close(config->is_async);
}

}  // extern "C"
