// sort.hip -- a stable sort of Fr columns by standard-form value, and on top of it the lookup
// argument's permuted pair (permute_expression_pair of a halo2-style prover: A' = the sorted input,
// S' = the table laid out beside it).  No reference counterpart: the reference keeps both on the CPU
// (a comparison sort and an ordered map) and uploads the four columns afterwards.
//
// The sort is an LSD radix sort of (32-bit key word, 32-bit index) pairs, one key word at a time:
//   k_sort_keys     the standard-form key of every element (from_mont when the input is Montgomery),
//                   stored as eight word planes, and the identity permutation;
//   k_sort_gather   word w of key[idx[i]] into a contiguous array -- the only random access per word;
//   four stable 8-bit passes over the pairs, each three plain launches:
//     k_sort_hist     per-workgroup digit histogram, and the digit totals of the pass;
//     k_sort_offsets  one workgroup per digit scans its row of the workgroups x 256 table;
//     k_sort_scatter  stable scatter: ranks within a wave by ballots, across waves by an LDS table
//                     of per-wave counts, across rounds by a running offset per digit.
// Four passes per word put the pairs back into the buffer they started in, so no buffer choice
// depends on a word having been skipped.  No workgroup ever waits for another one: no look-back, no
// flag another workgroup spins on, no cooperative launch (scan.hip states the rule and why).
//
// Batch.  All members ride in the same launches as ONE array of size * batch elements; the index is
// the element's position in that array.  After the eight key words the pairs are sorted once more,
// stably, by the member number idx / size (ceil(log256(batch)) passes, none for batch == 1), which
// brings every member's elements back together in sorted order.  This deviates from per-member
// offset tables on purpose: those need batch x workgroups x 256 words, which has no bound when the
// batch is many short members; the member passes cost one pass in 32 for up to 256 members and keep
// every table at workgroups x 256 whatever the batch.
//
// Uniform words.  Lookup columns are often small (range tables, bytes): the upper key words are the
// same in every element.  k_sort_keys sets varies[w] when some key differs from the first key in
// word w; the kernels of a word whose flag is clear return at once.  The flag is read on the device
// only (no host read-back), and skipping a whole word is the identity on the pairs.
//
// NOT constant time: digit bins, skipped words and the lookup's binary search depend on the values,
// as the MSM's bucket sort over witness scalars does.
#include <hip/hip_runtime.h>

#include "mbls_common.hpp"
#include "mbls_field.hpp"
#include "mbls_sort.hpp"

namespace mbls {

// ---- device helpers (the geometry, the scratch layout, match_digit, key_less and sort_key are
// mbls_sort.hpp's, shared with logup.hip)
// exclusive scan of one value per thread across the workgroup; `total` = the sum of all.
// sh: SORT_WAVES words, free again on return
MBLS_DEV uint32_t block_exscan(uint32_t v, uint32_t* sh, uint32_t& total) {
    const int lane = threadIdx.x & (SORT_WAVE - 1), wave = threadIdx.x / SORT_WAVE;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < SORT_WAVE; d <<= 1) {
        const uint32_t u = __shfl_up(inc, d, SORT_WAVE);
        if (lane >= d) inc += u;
    }
    if (lane == SORT_WAVE - 1) sh[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int j = 0; j < SORT_WAVES; ++j) {
        const uint32_t s = sh[j];
        before += j < wave ? s : 0u;
        total += s;
    }
    __syncthreads();
    return before + inc - v;
}

// element g of the call's array: the first n0 come from src0, the rest from src1
MBLS_DEV Fr sort_element(const uint8_t* src0, const uint8_t* src1, uint32_t n0, uint32_t g) {
    return load<FrCfg>(g < n0 ? src0 + 32 * (size_t)g : src1 + 32 * (size_t)(g - n0));
}

// ---- keys: planes[w * n + i] = word w of the standard-form key of element i, idx[i] = i
__global__ __launch_bounds__(SORT_THREADS) void k_sort_keys(uint32_t* __restrict__ planes, uint32_t* __restrict__ idx,
                                                            uint32_t* varies, const uint8_t* __restrict__ src0,
                                                            const uint8_t* __restrict__ src1, uint32_t n0, uint32_t n,
                                                            bool mont) {
    const uint32_t i = blockIdx.x * SORT_THREADS + threadIdx.x;
    if (i >= n) return;
    const Fr key = sort_key(sort_element(src0, src1, n0, i), mont);
#pragma unroll
    for (int w = 0; w < SORT_KEY_WORDS; ++w) planes[(size_t)w * n + i] = key.v[w];
    idx[i] = i;
    if constexpr (SORT_SKIP) {
        const Fr first = sort_key(load<FrCfg>(src0), mont);
#pragma unroll
        for (int w = 0; w < SORT_KEY_WORDS; ++w) {
            // every writer stores the same value; the read only spares most of the stores
            if (key.v[w] != first.v[w] && varies[w] == 0) varies[w] = 1;
        }
        if (i == 0) varies[SORT_KEY_WORDS] = 1;  // the member word: its pass count is the host's
    }
}

MBLS_DEV bool sort_skipped(const uint32_t* flag) {
    if constexpr (SORT_SKIP) return *flag == 0;
    return false;
}

// ---- the word of a round of passes: key word w, or the member number
__global__ __launch_bounds__(SORT_THREADS) void k_sort_gather(uint32_t* __restrict__ word, const uint32_t* __restrict__ idx,
                                                              const uint32_t* __restrict__ plane, uint32_t n,
                                                              const uint32_t* flag) {
    if (sort_skipped(flag)) return;
    const uint32_t i = blockIdx.x * SORT_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = idx[i];
    word[i] = g < n ? plane[g] : 0u;
}
__global__ __launch_bounds__(SORT_THREADS) void k_sort_member_word(uint32_t* __restrict__ word,
                                                                   const uint32_t* __restrict__ idx, uint32_t size,
                                                                   uint32_t n) {
    const uint32_t i = blockIdx.x * SORT_THREADS + threadIdx.x;
    if (i < n) word[i] = idx[i] / size;
}

// ---- launch 1 of a pass: hist[d * groups + grp] = elements of span grp with digit d;
// tot[d] += the same (tot is zero before the pass)
__global__ __launch_bounds__(SORT_THREADS) void k_sort_hist(uint32_t* __restrict__ hist, uint32_t* tot,
                                                            const uint32_t* __restrict__ word, int shift, SortGeom g,
                                                            const uint32_t* flag) {
    if (sort_skipped(flag)) return;
    __shared__ uint32_t cnt[SORT_DIGITS];
    const uint32_t t = threadIdx.x, lane = t & (SORT_WAVE - 1);
    cnt[t] = 0;
    __syncthreads();
    const uint32_t start = blockIdx.x * g.span;
    const uint32_t end = g.n - start < g.span ? g.n : start + g.span;
    for (uint32_t b = start; b < end; b += SORT_THREADS) {
        const bool valid = end - b > t;
        const uint32_t d = ((valid ? word[b + t] : 0u) >> shift) & (SORT_DIGITS - 1);
        const uint64_t peers = match_digit(d, valid);
        if (valid && (peers & ((1ull << lane) - 1)) == 0) atomicAdd(&cnt[d], (uint32_t)__popcll(peers));
    }
    __syncthreads();
    const uint32_t c = cnt[t];
    hist[(size_t)t * g.groups + blockIdx.x] = c;
    if (c) atomicAdd(&tot[t], c);
}

// ---- launch 2, one workgroup per digit d: hist[d * groups + grp] becomes the position of the first
// element of span grp with digit d: all smaller digits, then digit d in the earlier spans
__global__ __launch_bounds__(SORT_THREADS) void k_sort_offsets(uint32_t* __restrict__ hist, const uint32_t* __restrict__ tot,
                                                               uint32_t groups, const uint32_t* flag) {
    if (sort_skipped(flag)) return;
    __shared__ uint32_t sh[SORT_WAVES];
    const uint32_t d = blockIdx.x, t = threadIdx.x;
    uint32_t base, unused;
    block_exscan(t < d ? tot[t] : 0u, sh, base);
    uint32_t* row = hist + (size_t)d * groups;
    uint32_t x[SORT_SUMS_K], sum = 0;
#pragma unroll
    for (int k = 0; k < SORT_SUMS_K; ++k) {
        const uint32_t j = t * SORT_SUMS_K + k;
        x[k] = j < groups ? row[j] : 0u;
        sum += x[k];
    }
    uint32_t run = base + block_exscan(sum, sh, unused);
#pragma unroll
    for (int k = 0; k < SORT_SUMS_K; ++k) {
        const uint32_t j = t * SORT_SUMS_K + k;
        if (j < groups) row[j] = run;
        run += x[k];
    }
}

// ---- launch 3: the stable scatter.  A workgroup walks its span in rounds of SORT_THREADS elements
// in order; within a round the order is wave, then lane.
__global__ __launch_bounds__(SORT_THREADS) void k_sort_scatter(uint32_t* __restrict__ word_out, uint32_t* __restrict__ idx_out,
                                                               const uint32_t* __restrict__ word_in,
                                                               const uint32_t* __restrict__ idx_in,
                                                               const uint32_t* __restrict__ offsets, int shift, SortGeom g,
                                                               const uint32_t* flag) {
    if (sort_skipped(flag)) return;
    __shared__ uint32_t base[SORT_DIGITS];
    __shared__ uint32_t wc[SORT_WAVES][SORT_DIGITS];
    const uint32_t t = threadIdx.x, lane = t & (SORT_WAVE - 1), wave = t / SORT_WAVE;
    base[t] = offsets[(size_t)t * g.groups + blockIdx.x];
#pragma unroll
    for (int j = 0; j < SORT_WAVES; ++j) wc[j][t] = 0;
    __syncthreads();
    const uint32_t start = blockIdx.x * g.span;
    const uint32_t end = g.n - start < g.span ? g.n : start + g.span;
    bool valid = end - start > t;
    uint32_t w = valid ? word_in[start + t] : 0u, ix = valid ? idx_in[start + t] : 0u;
    for (uint32_t b = start; b < end; b += SORT_THREADS) {
        // the next round's pair, in flight over this round's barriers
        const uint32_t nb = b + SORT_THREADS;
        const bool nvalid = nb < end && end - nb > t;
        const uint32_t nw = nvalid ? word_in[nb + t] : 0u, nix = nvalid ? idx_in[nb + t] : 0u;
        const uint32_t d = (w >> shift) & (SORT_DIGITS - 1);
        const uint64_t peers = match_digit(d, valid);
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
        if (valid && rank == 0) wc[wave][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = base[d] + rank;
#pragma unroll
            for (int j = 0; j < SORT_WAVES; ++j) pos += (uint32_t)j < wave ? wc[j][d] : 0u;
            if (pos < g.n) {  // always, for a histogram of these same words
                word_out[pos] = w;
                idx_out[pos] = ix;
            }
        }
        __syncthreads();
        uint32_t s = 0;
#pragma unroll
        for (int j = 0; j < SORT_WAVES; ++j) {
            s += wc[j][t];
            wc[j][t] = 0;
        }
        base[t] += s;
        __syncthreads();
        valid = nvalid;
        w = nw;
        ix = nix;
    }
}

// ---- the outputs: row i of the sorted array is element idx[i].  Rows below n0 go to out0, the
// rest to out1 (either may be null); perm gets the index within the member, keys the standard form
__global__ __launch_bounds__(SORT_THREADS) void k_sort_emit(uint8_t* __restrict__ out0, uint8_t* __restrict__ out1,
                                                            uint32_t* __restrict__ perm, uint8_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ idx,
                                                            const uint8_t* __restrict__ src0,
                                                            const uint8_t* __restrict__ src1, uint32_t n0, uint32_t n,
                                                            uint32_t size, bool mont) {
    const uint32_t i = blockIdx.x * SORT_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t g = idx[i];
    if (g >= n) g = i;  // never, for a permutation
    if (perm) perm[i] = g % size;
    if (!out0 && !out1 && !keys) return;
    const Fr x = sort_element(src0, src1, n0, g);
    if (i < n0) {
        if (out0) store<FrCfg>(out0 + 32 * (size_t)i, x);
    } else if (out1) {
        store<FrCfg>(out1 + 32 * (size_t)(i - n0), x);
    }
    if (keys) store<FrCfg>(keys + 32 * (size_t)i, sort_key(x, mont));
}

// ---- the lookup match.  keys: the sorted standard-form keys, n0 input rows then n0 table rows,
// members of `size` rows in both halves.  flags (zero on entry, 2 n0 + 1 words): flags[i] = 1 for a
// repeated input row, flags[n0 + j] = 1 for a consumed table row; missing[k] counts the first rows
// of member k whose value the table lacks.
__global__ __launch_bounds__(SORT_THREADS) void k_lookup_flags(uint32_t* __restrict__ flags,
                                                               unsigned long long* __restrict__ missing,
                                                               const uint8_t* __restrict__ keys, uint32_t size,
                                                               uint32_t n0) {
    const uint32_t i = blockIdx.x * SORT_THREADS + threadIdx.x;
    if (i >= n0) return;
    const uint32_t k = i / size, r = i - k * size;
    const Fr a = load<FrCfg>(keys + 32 * (size_t)i);
    if (r != 0 && load<FrCfg>(keys + 32 * (size_t)(i - 1)) == a) {
        flags[i] = 1;
        return;
    }
    // the first entry of the member's sorted table that is not below a: at most 27 halvings of size <= 2^26
    const uint8_t* tab = keys + 32 * ((size_t)n0 + (size_t)k * size);
    uint32_t lo = 0, hi = size;
    for (int step = 0; step < 27 && lo < hi; ++step) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key_less(load<FrCfg>(tab + 32 * (size_t)mid), a)) lo = mid + 1;
        else hi = mid;
    }
    if (lo < size && load<FrCfg>(tab + 32 * (size_t)lo) == a) flags[n0 + k * size + lo] = 1;  // distinct values, distinct rows
    else atomicAdd(&missing[k], 1ull);
}

// ---- exclusive scan of `len` words in place, three launches in the scan skeleton's shape
__global__ __launch_bounds__(SORT_THREADS) void k_rank_reduce(uint32_t* __restrict__ sums, const uint32_t* __restrict__ v,
                                                              SortGeom g) {
    __shared__ uint32_t sh[SORT_WAVES];
    const uint32_t start = blockIdx.x * g.span;
    const uint32_t end = g.n - start < g.span ? g.n : start + g.span;
    uint32_t s = 0, total;
    for (uint32_t b = start; b < end; b += SORT_THREADS) s += end - b > threadIdx.x ? v[b + threadIdx.x] : 0u;
    block_exscan(s, sh, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(SORT_THREADS) void k_rank_sums(uint32_t* __restrict__ sums, uint32_t groups) {
    __shared__ uint32_t sh[SORT_WAVES];
    const uint32_t t = threadIdx.x;
    uint32_t x[SORT_SUMS_K], sum = 0, unused;
#pragma unroll
    for (int k = 0; k < SORT_SUMS_K; ++k) {
        const uint32_t j = t * SORT_SUMS_K + k;
        x[k] = j < groups ? sums[j] : 0u;
        sum += x[k];
    }
    uint32_t run = block_exscan(sum, sh, unused);
#pragma unroll
    for (int k = 0; k < SORT_SUMS_K; ++k) {
        const uint32_t j = t * SORT_SUMS_K + k;
        if (j < groups) sums[j] = run;
        run += x[k];
    }
}
__global__ __launch_bounds__(SORT_THREADS) void k_rank_write(uint32_t* v, const uint32_t* __restrict__ sums, SortGeom g) {
    __shared__ uint32_t sh[SORT_WAVES];
    const uint32_t start = blockIdx.x * g.span;
    const uint32_t end = g.n - start < g.span ? g.n : start + g.span;
    uint32_t run = sums[blockIdx.x];
    for (uint32_t b = start; b < end; b += SORT_TILE) {
        const uint32_t at = b + threadIdx.x * SORT_K;  // < 2^28: no wrap
        uint32_t x[SORT_K], sum = 0, total;
#pragma unroll
        for (int k = 0; k < SORT_K; ++k) {
            x[k] = at + k < end ? v[at + k] : 0u;
            sum += x[k];
        }
        uint32_t cur = run + block_exscan(sum, sh, total);
#pragma unroll
        for (int k = 0; k < SORT_K; ++k) {
            if (at + k < end) v[at + k] = cur;
            cur += x[k];
        }
        run += total;
    }
}

// ---- left[k * size + q] = the q-th unconsumed row of member k's sorted table.  S: the scanned flags
__global__ __launch_bounds__(SORT_THREADS) void k_lookup_compact(uint32_t* __restrict__ left, const uint32_t* __restrict__ S,
                                                                 uint32_t size, uint32_t n0) {
    const uint32_t j = blockIdx.x * SORT_THREADS + threadIdx.x;
    if (j >= n0) return;
    const uint32_t k = j / size, r = j - k * size;
    const uint32_t here = S[n0 + j];
    if (S[n0 + j + 1] != here) return;  // consumed
    const uint32_t q = r - (here - S[n0 + k * size]);
    if (q < size) left[k * size + q] = r;
}

// ---- S'[i] = A'[i] on a first row; the repeated rows R_0 < R_1 < .. of a member take the member's
// leftovers from the back: S'[R_q] = L[m - 1 - q]
__global__ __launch_bounds__(SORT_THREADS) void k_lookup_write(uint8_t* __restrict__ ptab, const uint8_t* __restrict__ pin,
                                                               const uint8_t* __restrict__ tsorted,
                                                               const uint32_t* __restrict__ left,
                                                               const uint32_t* __restrict__ S, uint32_t size, uint32_t n0) {
    const uint32_t i = blockIdx.x * SORT_THREADS + threadIdx.x;
    if (i >= n0) return;
    const uint32_t here = S[i];
    const uint8_t* from = pin + 32 * (size_t)i;
    if (S[i + 1] != here) {
        const uint32_t k = i / size, s0 = S[k * size];
        const uint32_t q = here - s0, m = S[(k + 1) * size] - s0;
        uint32_t slot = m - 1 - q;
        if (slot >= size) slot = 0;  // never: q < m <= size
        uint32_t row = left[k * size + slot];
        if (row >= size) row = 0;    // never: the leftovers number at least m
        from = tsorted + 32 * ((size_t)k * size + row);
    }
    store<FrCfg>(ptab + 32 * (size_t)i, load<FrCfg>(from));
}

// ---- host side
// Sorts the g.n elements src0[0 .. n0) ++ src1[0 .. n - n0), members of `size`; returns the buffer
// holding the sorted permutation (global indices) in *idx_out.
eIcicleError sort_launch(const SortGeom& g, size_t size, uint8_t* scratch, const SortLayout& L, const uint8_t* src0,
                         const uint8_t* src1, uint32_t n0, bool mont, hipStream_t st, const uint32_t** idx_out) {
    const uint32_t n = g.n;
    uint32_t* planes = reinterpret_cast<uint32_t*>(scratch + L.planes);
    uint32_t* word[2] = {reinterpret_cast<uint32_t*>(scratch + L.word_a), reinterpret_cast<uint32_t*>(scratch + L.word_b)};
    uint32_t* idx[2] = {reinterpret_cast<uint32_t*>(scratch + L.idx_a), reinterpret_cast<uint32_t*>(scratch + L.idx_b)};
    uint32_t* hist = reinterpret_cast<uint32_t*>(scratch + L.hist);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(scratch + L.ctl);
    uint32_t* varies = ctl + SORT_CTL_VARIES;
    const dim3 block(SORT_THREADS), per_elem(sort_blocks(n)), per_span(g.groups);
    MBLS_TRY(hipMemsetAsync(ctl, 0, 4 * SORT_CTL_WORDS, st));
    hipLaunchKernelGGL(k_sort_keys, per_elem, block, 0, st, planes, idx[0], varies, src0, src1, n0, n, mont);
    int pass = 0, cur = 0;
    auto digit_pass = [&](int shift, const uint32_t* flag) {
        uint32_t* tot = ctl + (size_t)pass * SORT_DIGITS;
        hipLaunchKernelGGL(k_sort_hist, per_span, block, 0, st, hist, tot, word[cur], shift, g, flag);
        hipLaunchKernelGGL(k_sort_offsets, dim3(SORT_DIGITS), block, 0, st, hist, tot, g.groups, flag);
        hipLaunchKernelGGL(k_sort_scatter, per_span, block, 0, st, word[cur ^ 1], idx[cur ^ 1], word[cur], idx[cur], hist,
                           shift, g, flag);
        cur ^= 1;
        ++pass;
    };
    for (int w = 0; w < SORT_KEY_WORDS; ++w) {
        hipLaunchKernelGGL(k_sort_gather, per_elem, block, 0, st, word[cur], idx[cur], planes + (size_t)w * n, n, varies + w);
        for (int p = 0; p < SORT_WORD_PASSES; ++p) digit_pass(p * SORT_BITS, varies + w);
    }
    const int member_passes = sort_member_passes(n / size);
    if (member_passes) {
        hipLaunchKernelGGL(k_sort_member_word, per_elem, block, 0, st, word[cur], idx[cur], (uint32_t)size, n);
        for (int p = 0; p < member_passes; ++p) digit_pass(p * SORT_BITS, varies + SORT_KEY_WORDS);
    }
    MBLS_TRY(hipGetLastError());
    *idx_out = idx[cur];
    return MBLS_SUCCESS;
}

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError mbls_fr_sort(const mbls_fr_t* input, size_t size, bool montgomery, const VecOpsConfig* config, mbls_fr_t* sorted,
                          uint32_t* perm) {
    if (!input || !config || (!sorted && !perm)) return MBLS_INVALID_POINTER;
    SortCall c;
    eIcicleError er = sort_call(size, config, &c);
    if (er != MBLS_SUCCESS) return er;
    hipStream_t st = static_cast<hipStream_t>(config->stream);
    const size_t n = c.size * c.batch;
    const SortGeom g = sort_geom(n);
    const SortLayout L = sort_layout(n, false, c.batch);

    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *scratch, *dsorted = nullptr, *dperm = nullptr;
    const uint8_t* din;
    S.scratch(&scratch, L.bytes);
    S.in(&din, input, 32 * n, config->is_a_on_device);
    if (sorted) S.out(&dsorted, sorted, 32 * n, config->is_result_on_device);
    if (perm) S.out(&dperm, perm, 4 * n, config->is_result_on_device);
    er = S.open();
    if (er != MBLS_SUCCESS) return er;
    const uint32_t* idx;
    er = sort_launch(g, c.size, scratch, L, din, nullptr, g.n, montgomery, st, &idx);
    if (er != MBLS_SUCCESS) return er;
    hipLaunchKernelGGL(k_sort_emit, dim3(sort_blocks(n)), dim3(SORT_THREADS), 0, st, dsorted, (uint8_t*)nullptr,
                       reinterpret_cast<uint32_t*>(dperm), (uint8_t*)nullptr, idx, din, (const uint8_t*)nullptr, g.n, g.n,
                       (uint32_t)c.size, montgomery);
    MBLS_TRY(hipGetLastError());
    return S.close(config->is_async);
}

eIcicleError mbls_fr_lookup_permute(const mbls_fr_t* input, const mbls_fr_t* table, size_t size, bool montgomery,
                                    const VecOpsConfig* config, mbls_fr_t* permuted_input, mbls_fr_t* permuted_table,
                                    uint64_t* n_missing) {
    if (!input || !table || !config || !permuted_input || !permuted_table) return MBLS_INVALID_POINTER;
    SortCall c;
    eIcicleError er = sort_call(size, config, &c);
    if (er != MBLS_SUCCESS) return er;
    hipStream_t st = static_cast<hipStream_t>(config->stream);
    const size_t n0 = c.size * c.batch, n = 2 * n0;
    const SortGeom g = sort_geom(n), gr = sort_geom(n + 1);
    const SortLayout L = sort_layout(n, true, c.batch);

    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *scratch, *dpin, *dptab;
    const uint8_t *din, *dtab;
    S.scratch(&scratch, L.bytes);
    S.in(&din, input, 32 * n0, config->is_a_on_device);
    S.in(&dtab, table, 32 * n0, config->is_a_on_device);
    S.out(&dpin, permuted_input, 32 * n0, config->is_result_on_device);
    S.out(&dptab, permuted_table, 32 * n0, config->is_result_on_device);
    er = S.open();
    if (er != MBLS_SUCCESS) return er;
    const uint32_t* idx;
    er = sort_launch(g, c.size, scratch, L, din, dtab, (uint32_t)n0, montgomery, st, &idx);
    if (er != MBLS_SUCCESS) return er;
    // the planes are done with: the sorted keys take their place
    uint8_t *keys = scratch + L.planes, *tsorted = scratch + L.tsorted;
    uint32_t* flags = reinterpret_cast<uint32_t*>(scratch + L.flags);
    uint32_t* sums = reinterpret_cast<uint32_t*>(scratch + L.sums);
    uint32_t* left = reinterpret_cast<uint32_t*>(scratch + L.left);
    unsigned long long* missing = reinterpret_cast<unsigned long long*>(scratch + L.missing);
    const dim3 block(SORT_THREADS), per_row(sort_blocks(n0));
    const uint32_t size32 = (uint32_t)c.size, rows = (uint32_t)n0;
    MBLS_TRY(hipMemsetAsync(flags, 0, 4 * (n + 1), st));
    MBLS_TRY(hipMemsetAsync(missing, 0, 8 * c.batch, st));
    hipLaunchKernelGGL(k_sort_emit, dim3(sort_blocks(n)), block, 0, st, dpin, tsorted, (uint32_t*)nullptr, keys, idx, din,
                       dtab, rows, g.n, size32, montgomery);
    hipLaunchKernelGGL(k_lookup_flags, per_row, block, 0, st, flags, missing, keys, size32, rows);
    hipLaunchKernelGGL(k_rank_reduce, dim3(gr.groups), block, 0, st, sums, flags, gr);
    hipLaunchKernelGGL(k_rank_sums, dim3(1), block, 0, st, sums, gr.groups);
    hipLaunchKernelGGL(k_rank_write, dim3(gr.groups), block, 0, st, flags, sums, gr);
    hipLaunchKernelGGL(k_lookup_compact, per_row, block, 0, st, left, flags, size32, rows);
    hipLaunchKernelGGL(k_lookup_write, per_row, block, 0, st, dptab, dpin, tsorted, left, flags, size32, rows);
    MBLS_TRY(hipGetLastError());
    if (n_missing) MBLS_TRY(hipMemcpyAsync(n_missing, missing, 8 * c.batch, hipMemcpyDeviceToHost, st));
    return S.close(config->is_async && !n_missing);
}

eIcicleError mbls_fr_sort_plan(size_t size, int batch, int64_t* out) {
    if (!out) return MBLS_INVALID_POINTER;
    if (size == 0 || batch < 1 || size > SORT_MAX_ELEMS || size * (size_t)batch > SORT_MAX_ELEMS) return MBLS_INVALID_ARGUMENT;
    const size_t n = size * (size_t)batch;
    const SortGeom g = sort_geom(n);
    out[0] = SORT_BITS;
    out[1] = SORT_KEY_WORDS * SORT_WORD_PASSES + sort_member_passes((size_t)batch);
    out[2] = SORT_TILE;
    out[3] = g.groups;
    out[4] = (int64_t)sort_layout(n, false, (size_t)batch).bytes;
    out[5] = (int64_t)sort_layout(2 * n, true, (size_t)batch).bytes;
    return MBLS_SUCCESS;
}

}  // extern "C"
