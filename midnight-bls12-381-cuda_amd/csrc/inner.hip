// inner.hip -- Fr inner products of columns with vectors, out[p][k] = sum_i columns[p][i] * vectors[k][i],
// the multi-point polynomial evaluation built on them (the vectors are the powers of the points) and
// the fill of a column with init * base^i.  No reference counterpart: the reference evaluates its
// polynomials on the CPU (eval_polynomial), one Horner pass per (polynomial, point) pair.
//
// Shape.  Two plain launches, no workgroup waits for another, no atomics.  k_inner: a workgroup owns
// a block of INNER_CB columns x INNER_VB vectors and a run of consecutive tiles of the rows; a thread
// loads the CB + VB elements of a row once and forms the CB * VB products from registers.  Each
// workgroup writes one partial sum per (column, vector) of its block; k_inner_fold adds the partial
// sums of an output -- their number is bounded by the plan (mbls_inner.hpp), not by `size`.
//
// Deferred reduction.  The products are radix-2^29 (mbls_fr29.hpp): 9 limbs < 2^29 per operand (the
// top one < 2^24, the operands being words < 2^256), 17 product columns.  Column k of one product
// is a sum of at most 9 limb products, each <= (2^29 - 1)^2 < 2^58, so it is < 9 * 2^58.  A thread
// adds the columns of INNER_DEFER = 7 products into ONE 64-bit accumulator per column before it
// reduces:
//     7 * 9 * 2^58 = 63 * 2^58 < 2^64,
// and the carry sweep that normalises the columns adds a carry < 2^35 to a column < 63 * 2^58, still
// < 2^64.  (8 products would need 72 * 2^58 > 2^64.)  The value is then T = sum of 7 products of
// canonical operands, T < 7 r^2 < 2^513: 18 normalised limbs, and ONE Montgomery reduction by
// 2^261 gives (T + m r) / 2^261 < 7 r^2 / 2^261 + r < r (1 + 7/64) < 2r, canonical after one
// conditional subtraction.  tests/inner_model.py restates the accumulation and asserts the column
// bound; the all-(r - 1) case of tests/test_gpu_inner.py drives 7 maximal products into every column.
//
// Montgomery factors: operands are a R, b R (R = 2^256), the reduction divides by 2^261, so the
// partial sums hold S R / 32; k_inner_fold doubles five times.
//
// The columns are witness polynomials: no branch and no address below depends on a field value; the
// conditions are on thread, block, row index and the counts only.  The powers kernels branch on the
// bits of a row index, never on the base.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "mbls_common.hpp"
#include "mbls_field.hpp"
#include "mbls_fr29.hpp"
#include "mbls_inner.hpp"

namespace mbls {

static constexpr int INNER_NCOL = 2 * r29::NL - 1;  // 17 product columns
static_assert((uint64_t)INNER_DEFER * 9 <= 63, "deferred columns: DEFER * 9 * 2^58 must stay below 2^64");

// acc[k] += sum_{i + j = k} a_i b_j, one v_mad_u64_u32 chain per column, no reduction
template <int K>
MBLS_DEV void inner_mac_cols(uint64_t (&acc)[INNER_NCOL], const r29::F29& a, const r29::F29& b) {
    if constexpr (K < INNER_NCOL) {
        constexpr int LO = K > r29::NL - 1 ? K - (r29::NL - 1) : 0;
        madc::col<K, LO, (K < r29::NL - 1 ? K : r29::NL - 1), false>(acc[K], a.l, b.l);
        inner_mac_cols<K + 1>(acc, a, b);
    }
}

// Montgomery reduction by 2^261 of normalised limbs t[0..17] (value < 2^513): mul_cols of
// mbls_fr29.hpp with the limb products replaced by the limbs themselves
template <int K>
MBLS_DEV void inner_red_cols(uint64_t& acc, uint32_t (&m)[r29::NL], r29::F29& r, const uint32_t (&t)[INNER_NCOL + 1]) {
    using namespace r29;
    if constexpr (K < INNER_NCOL) {
        constexpr int LO = K > NL - 1 ? K - (NL - 1) : 0;
        acc += t[K];
        madc::col<K, LO, (K < NL ? K : NL) - 1, true>(acc, m, RL);
        if constexpr (K < NL) {
            m[K] = (0u - (uint32_t)acc) & MASK;
            acc += m[K];
        } else {
            r.l[K - NL] = (uint32_t)acc & MASK;
        }
        acc >>= 29;
        inner_red_cols<K + 1>(acc, m, r, t);
    }
}

// the unreduced columns of <= INNER_DEFER products -> the canonical value T / 2^261 mod r
MBLS_DEV Fr inner_reduce(const uint64_t (&cols)[INNER_NCOL]) {
    uint32_t t[INNER_NCOL + 1];
    uint64_t carry = 0;
#pragma unroll
    for (int k = 0; k < INNER_NCOL; ++k) {
        const uint64_t s = cols[k] + carry;  // < 63 * 2^58 + 2^35 < 2^64
        t[k] = (uint32_t)s & r29::MASK;
        carry = s >> 29;
    }
    t[INNER_NCOL] = (uint32_t)carry;  // T < 2^513: the carry is limb 17, below 2^20
    uint32_t m[r29::NL];
    r29::F29 r;
    uint64_t acc = 0;
    inner_red_cols<0>(acc, m, r, t);
    r.l[r29::NL - 1] = (uint32_t)acc + t[INNER_NCOL];
    Fr x = r29::pack(r);
    reduce_once(x);
    return x;
}

// sum over the workgroup's 256 threads, valid in thread 0; lds: 8 * 256 words, word-major
MBLS_DEV Fr inner_block_sum(Fr x, uint32_t* lds) {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int w = 0; w < 8; ++w) lds[w * INNER_THREADS + tid] = x.v[w];
    __syncthreads();
    for (uint32_t s = INNER_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            Fr y;
#pragma unroll
            for (int w = 0; w < 8; ++w) y.v[w] = lds[w * INNER_THREADS + tid + s];
            x = x + y;
#pragma unroll
            for (int w = 0; w < 8; ++w) lds[w * INNER_THREADS + tid] = x.v[w];
        }
        __syncthreads();
    }
    return x;
}

// partial[((c * n_vecs + v) * groups + g)] = sum over the rows of group g of cols[c][i] * vecs[v][i],
// as S R / 32.  grid: groups * ncb * nvb workgroups, the blocks of one row group next to each other
// so that the vector elements they share meet in L2.
template <int CB, int VB>
__global__ __launch_bounds__(INNER_THREADS) void k_inner(uint8_t* __restrict__ partial,
                                                          const uint8_t* const* __restrict__ cols,
                                                          const uint8_t* const* __restrict__ vecs, uint32_t n_cols,
                                                          uint32_t n_vecs, size_t size, uint32_t ncb, uint32_t nvb,
                                                          uint32_t tiles_per_group, uint32_t groups) {
    __shared__ uint32_t lds[8 * INNER_THREADS];
    const uint32_t tid = threadIdx.x, bid = blockIdx.x;
    const uint32_t vbi = bid % nvb, cbi = (bid / nvb) % ncb, g = bid / (nvb * ncb);
    const uint32_t c0 = cbi * CB, v0 = vbi * VB;
    const uint32_t nc = n_cols - c0 < (uint32_t)CB ? n_cols - c0 : (uint32_t)CB;
    const uint32_t nv = n_vecs - v0 < (uint32_t)VB ? n_vecs - v0 : (uint32_t)VB;
    const uint8_t* cp[CB];
    const uint8_t* vp[VB];
#pragma unroll
    for (int c = 0; c < CB; ++c) cp[c] = cols[c0 + ((uint32_t)c < nc ? c : 0)];
#pragma unroll
    for (int v = 0; v < VB; ++v) vp[v] = vecs[v0 + ((uint32_t)v < nv ? v : 0)];

    const size_t row0 = (size_t)g * tiles_per_group * INNER_TILE;
    const size_t span_end = row0 + (size_t)tiles_per_group * INNER_TILE;
    const size_t end = span_end < size ? span_end : size;

    Fr run[CB][VB], na[CB], nb[VB];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        na[c] = Fr::zero();
#pragma unroll
        for (int v = 0; v < VB; ++v) run[c][v] = Fr::zero();
    }
#pragma unroll
    for (int v = 0; v < VB; ++v) nb[v] = Fr::zero();

    // the next row's operands are in flight while this row's products run
    size_t i = row0 + tid;
    if (i < end) {
#pragma unroll
        for (int c = 0; c < CB; ++c)
            if ((uint32_t)c < nc) na[c] = load<FrCfg>(cp[c] + 32 * i);
#pragma unroll
        for (int v = 0; v < VB; ++v)
            if ((uint32_t)v < nv) nb[v] = load<FrCfg>(vp[v] + 32 * i);
    }
    for (uint32_t t = 0; t < tiles_per_group; ++t) {
        uint64_t acc[CB][VB][INNER_NCOL];
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
            for (int v = 0; v < VB; ++v)
#pragma unroll
                for (int k = 0; k < INNER_NCOL; ++k) acc[c][v][k] = 0;
#pragma unroll 1
        for (int j = 0; j < INNER_DEFER; ++j) {
            Fr a[CB];
            r29::F29 b[VB];
#pragma unroll
            for (int c = 0; c < CB; ++c) a[c] = na[c];
#pragma unroll
            for (int v = 0; v < VB; ++v) b[v] = r29::unpack(nb[v]);
            const size_t inext = i + INNER_THREADS;
            if (inext < end) {
#pragma unroll
                for (int c = 0; c < CB; ++c)
                    if ((uint32_t)c < nc) na[c] = load<FrCfg>(cp[c] + 32 * inext);
#pragma unroll
                for (int v = 0; v < VB; ++v)
                    if ((uint32_t)v < nv) nb[v] = load<FrCfg>(vp[v] + 32 * inext);
            }
            if (i < end) {
#pragma unroll
                for (int c = 0; c < CB; ++c) {
                    if ((uint32_t)c < nc) {
                        const r29::F29 al = r29::unpack(a[c]);
#pragma unroll
                        for (int v = 0; v < VB; ++v)
                            if ((uint32_t)v < nv) inner_mac_cols<0>(acc[c][v], al, b[v]);
                    }
                }
            }
            i = inext;
        }
        // one reduction for the tile's <= INNER_DEFER products per pair
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
            for (int v = 0; v < VB; ++v)
                if ((uint32_t)c < nc && (uint32_t)v < nv) run[c][v] = run[c][v] + inner_reduce(acc[c][v]);
    }
#pragma unroll
    for (int c = 0; c < CB; ++c) {
#pragma unroll
        for (int v = 0; v < VB; ++v) {
            if ((uint32_t)c < nc && (uint32_t)v < nv) {  // uniform over the workgroup
                const Fr s = inner_block_sum(run[c][v], lds);
                if (tid == 0)
                    store<FrCfg>(partial + 32 * (((size_t)(c0 + c) * n_vecs + (v0 + v)) * groups + g), s);
            }
        }
    }
}

// out[pair] = 32 * sum_g partial[pair * groups + g], canonical.  One workgroup per output.
__global__ __launch_bounds__(INNER_THREADS) void k_inner_fold(uint8_t* __restrict__ out, const uint8_t* __restrict__ partial,
                                                               uint32_t groups) {
    __shared__ uint32_t lds[8 * INNER_THREADS];
    const size_t pair = blockIdx.x;
    Fr x = Fr::zero();
    for (uint32_t g = threadIdx.x; g < groups; g += INNER_THREADS) x = x + load<FrCfg>(partial + 32 * (pair * groups + g));
    x = inner_block_sum(x, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) x = dbl(x);
        store<FrCfg>(out + 32 * pair, x);
    }
}

// ---- powers: base^i = hi[i >> s] * lo[i & (2^s - 1)], hi[j] = init * base^(j 2^s), lo[j] = base^j.
// The tables hold about 2 sqrt(size) entries per member, each by square-and-multiply over the bits of
// its INDEX (public); the fill is one product per element.  x^0 = 1 for every x, 0 included.
MBLS_DEV Fr inner_pow_index(const Fr& x, uint32_t e) {
    Fr acc = Fr::one();
    for (int b = 31 - __builtin_clz(e | 1u); b >= 0; --b) {
        acc = sqr(acc);
        if ((e >> b) & 1u) acc = acc * x;
    }
    return acc;
}
// tab: per member k, lo at tab + 32 * k * (nlo + nhi), hi right after it
__global__ __launch_bounds__(256) void k_pow_tables(uint8_t* __restrict__ tab, const uint8_t* __restrict__ base,
                                                    const uint8_t* __restrict__ init, uint32_t s, uint32_t nhi,
                                                    size_t total) {
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint32_t nlo = 1u << s, per = nlo + nhi;
    const size_t k = idx / per;
    const uint32_t j = (uint32_t)(idx % per);
    Fr x = load<FrCfg>(base + 32 * k), y;
    if (j < nlo) {
        y = inner_pow_index(x, j);
    } else {
        for (uint32_t q = 0; q < s; ++q) x = sqr(x);
        y = inner_pow_index(x, j - nlo);
        if (init) y = y * load<FrCfg>(init + 32 * k);
    }
    store<FrCfg>(tab + 32 * idx, y);
}
__global__ __launch_bounds__(256) void k_pow_fill(uint8_t* __restrict__ out, const uint8_t* __restrict__ tab, size_t size,
                                                  uint32_t s, uint32_t nhi, size_t total) {
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint32_t nlo = 1u << s;
    const size_t k = idx / size, i = idx % size;
    const uint8_t* t = tab + 32 * k * ((size_t)nlo + nhi);
    const Fr lo = load<FrCfg>(t + 32 * (i & (nlo - 1))), hi = load<FrCfg>(t + 32 * ((size_t)nlo + (i >> s)));
    store<FrCfg>(out + 32 * idx, hi * lo);
}

static void powers_launch(uint8_t* out, uint8_t* tab, const uint8_t* base, const uint8_t* init, size_t size, size_t batch,
                          const InnerGeom& g, hipStream_t st) {
    const size_t entries = batch * (g.pow_lo + g.pow_hi), total = batch * size;
    hipLaunchKernelGGL(k_pow_tables, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, tab, base, init,
                       (uint32_t)g.pow_log, (uint32_t)g.pow_hi, entries);
    hipLaunchKernelGGL(k_pow_fill, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out, tab, size,
                       (uint32_t)g.pow_log, (uint32_t)g.pow_hi, total);
}

// the two launches over device operands; dtab: the device block for the pointer tables
static eIcicleError inner_launch(const std::vector<const uint8_t*>& ptrs, int n_columns, int n_vectors, size_t size,
                                 const InnerGeom& g, uint8_t* dtab, uint8_t* partial, uint8_t* out, hipStream_t st) {
    // the copy leaves pageable memory before hipMemcpyAsync returns, as the staged operands do
    MBLS_TRY(hipMemcpyAsync(dtab, ptrs.data(), sizeof(void*) * ptrs.size(), hipMemcpyHostToDevice, st));
    const uint8_t* const* dcols = reinterpret_cast<const uint8_t* const*>(dtab);
    hipLaunchKernelGGL((k_inner<INNER_CB, INNER_VB>), dim3(g.groups * g.ncb * g.nvb), dim3(INNER_THREADS), 0, st, partial,
                       dcols, dcols + n_columns, (uint32_t)n_columns, (uint32_t)n_vectors, size, g.ncb, g.nvb,
                       g.tiles_per_group, g.groups);
    hipLaunchKernelGGL(k_inner_fold, dim3((unsigned)(n_columns * n_vectors)), dim3(INNER_THREADS), 0, st, out, partial,
                       g.groups);
    MBLS_TRY(hipGetLastError());
    return MBLS_SUCCESS;
}

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError mbls_fr_inner_products(const mbls_fr_t* const* columns, int n_columns, const mbls_fr_t* const* vectors,
                                    int n_vectors, size_t size, const VecOpsConfig* config, mbls_fr_t* output) {
    if (!columns || !vectors || !config || !output) return MBLS_INVALID_POINTER;
    if (size == 0 || size > INNER_MAX_ROWS) return MBLS_INVALID_ARGUMENT;
    eIcicleError er = check_table(columns, n_columns, INNER_MAX_COLUMNS);
    if (er != MBLS_SUCCESS) return er;
    er = check_table(vectors, n_vectors, INNER_MAX_VECTORS);
    if (er != MBLS_SUCCESS) return er;
    hipStream_t st = static_cast<hipStream_t>(config->stream);
    const InnerGeom g = inner_geom(size, n_columns, n_vectors);
    static thread_local std::vector<const uint8_t*> ptrs;
    ptrs.resize((size_t)(n_columns + n_vectors));

    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *scratch, *dout;
    // the partial sums, then the pointer tables
    S.scratch(&scratch, g.partial_bytes + g.table_bytes);
    S.in_table(ptrs.data(), columns, n_columns, 32 * size, config->is_a_on_device);
    S.in_table(ptrs.data() + n_columns, vectors, n_vectors, 32 * size, config->is_b_on_device);
    S.out(&dout, output, 32 * (size_t)n_columns * (size_t)n_vectors, config->is_result_on_device);
    er = S.open();
    if (er != MBLS_SUCCESS) return er;
    er = inner_launch(ptrs, n_columns, n_vectors, size, g, scratch + g.partial_bytes, scratch, dout, st);
    if (er != MBLS_SUCCESS) return er;
    return S.close(config->is_async);
}

eIcicleError mbls_fr_multi_eval(const mbls_fr_t* const* columns, int n_columns, size_t size, const mbls_fr_t* points,
                                int n_points, const VecOpsConfig* config, mbls_fr_t* output) {
    if (!columns || !points || !config || !output) return MBLS_INVALID_POINTER;
    if (size == 0 || size > INNER_MAX_ROWS) return MBLS_INVALID_ARGUMENT;
    eIcicleError er = check_table(columns, n_columns, INNER_MAX_COLUMNS);
    if (er != MBLS_SUCCESS) return er;
    if (n_points < 1 || n_points > INNER_MAX_VECTORS) return MBLS_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(config->stream);
    const InnerGeom g = inner_geom(size, n_columns, n_points);
    const size_t col_bytes = 32 * size, tab_bytes = inner_pow_table_bytes(g, (size_t)n_points);
    static thread_local std::vector<const uint8_t*> ptrs;
    ptrs.resize((size_t)(n_columns + n_points));

    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *scratch, *dout;
    const uint8_t* dpoints;
    // the partial sums, the pointer tables, the power tables, then the powers of every point
    S.scratch(&scratch, g.partial_bytes + g.table_bytes + tab_bytes + align_up(col_bytes * (size_t)n_points));
    S.in_table(ptrs.data(), columns, n_columns, col_bytes, config->is_a_on_device);
    S.in(&dpoints, points, 32 * (size_t)n_points, config->is_b_on_device);
    S.out(&dout, output, 32 * (size_t)n_columns * (size_t)n_points, config->is_result_on_device);
    er = S.open();
    if (er != MBLS_SUCCESS) return er;
    uint8_t* dtab = scratch + g.partial_bytes;
    uint8_t* ptab = dtab + g.table_bytes;
    uint8_t* pw = ptab + tab_bytes;
    // the powers of the points, a batch of n_points members: vector k starts at row k * size
    powers_launch(pw, ptab, dpoints, nullptr, size, (size_t)n_points, g, st);
    for (int k = 0; k < n_points; ++k) ptrs[(size_t)(n_columns + k)] = pw + col_bytes * (size_t)k;
    er = inner_launch(ptrs, n_columns, n_points, size, g, dtab, scratch, dout, st);
    if (er != MBLS_SUCCESS) return er;
    return S.close(config->is_async);
}

eIcicleError mbls_fr_powers(const mbls_fr_t* base, const mbls_fr_t* init, size_t size, const VecOpsConfig* config,
                            mbls_fr_t* output) {
    if (!base || !config || !output) return MBLS_INVALID_POINTER;
    if (config->columns_batch) return MBLS_API_NOT_IMPLEMENTED;
    const size_t batch = config->batch_size > 0 ? (size_t)config->batch_size : 1;
    if (size == 0 || size > INNER_MAX_ROWS || size * batch > INNER_MAX_ROWS) return MBLS_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(config->stream);
    const InnerGeom g = inner_geom(size, 1, 1);

    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *tab, *dout;
    const uint8_t *dbase, *dinit = nullptr;
    S.scratch(&tab, inner_pow_table_bytes(g, batch));
    S.in(&dbase, base, 32 * batch, config->is_b_on_device);
    if (init) S.in(&dinit, init, 32 * batch, config->is_b_on_device);
    S.out(&dout, output, 32 * size * batch, config->is_result_on_device);
    eIcicleError er = S.open();
    if (er != MBLS_SUCCESS) return er;
    powers_launch(dout, tab, dbase, dinit, size, batch, g, st);
    MBLS_TRY(hipGetLastError());
    return S.close(config->is_async);
}

eIcicleError mbls_fr_inner_plan(size_t size, int n_columns, int n_vectors, int64_t* out) {
    if (!out) return MBLS_INVALID_POINTER;
    if (size == 0 || size > INNER_MAX_ROWS || n_columns < 1 || n_columns > INNER_MAX_COLUMNS || n_vectors < 1 ||
        n_vectors > INNER_MAX_VECTORS)
        return MBLS_INVALID_ARGUMENT;
    const InnerGeom g = inner_geom(size, n_columns, n_vectors);
    const size_t inner = g.partial_bytes + g.table_bytes;
    out[0] = INNER_TILE;
    out[1] = INNER_DEFER;
    out[2] = INNER_CB;
    out[3] = INNER_VB;
    out[4] = (int64_t)std::max<uint32_t>(INNER_TARGET_WGS, g.ncb * g.nvb);
    out[5] = g.group_cap;
    out[6] = g.tiles_per_group;
    out[7] = g.groups;
    out[8] = (int64_t)g.groups * g.ncb * g.nvb;
    out[9] = (int64_t)inner;
    out[10] = (int64_t)(inner + inner_pow_table_bytes(g, (size_t)n_vectors) + align_up(32 * size * (size_t)n_vectors));
    out[11] = g.pow_log;
    return MBLS_SUCCESS;
}

}  // extern "C"
