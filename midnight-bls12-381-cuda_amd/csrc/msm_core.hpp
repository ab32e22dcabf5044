// msm_core.hpp -- Pippenger multi-scalar multiplication over G1 / G2 for CDNA4 (templates).
//
// Reference: orchestration msm::msm_cuda (bls12-381/src/curve/msm_kernels.cu:603-903),
// digits compute_bucket_indices_kernel (:69-143), histogram (:224-256), cub scan+sort
// (:748-781), accumulation (:269-366), bucket reduction (:376-513), final (:529-596);
// boundary msm_cuda_impl / msm_g2_cuda_impl (icicle_curve_api.cu:243-618).
//
// Pipeline (all on the caller's stream; scratch: one region of the leased arena, laid out by
// msm_scratch below -- the one list of its blocks, used both to size and to carve it):
//   1-3. the front (msm_front, msm_common.hip; one front serves G1 and G2): signed c-bit digits
//                     of each scalar (Montgomery -> standard if flagged, endomorphism split with
//                     its per-call image table), contributions (index|sign) sorted by bucket.
//                     c <= 16 (default, and every split plan): the partitioned counting sort,
//                     k_digits_part + k_part_sort.  Unsplit c > 16: k_digits (key, value pairs,
//                     bucket histogram by atomics), scans, k_scatter.  Then k_chunk_counts / k_chunk_owner: buckets
//                     are split in chunks of <= P.chunk points so one heavy bucket (e.g.
//                     all-equal scalars) cannot serialise a thread.
//   4. k_accumulate_r28 (G1) / k_accumulate_r28p (G2): one thread (lane pair) per chunk, sum of
//                     +-P_i by mixed additions in radix-2^28 XYZZ -> raw XYZZ partial.
//   5. k_bucket_small one thread (lane pair) per light bucket: sum of its chunk partials; heavy
//                     buckets (> SMALL_MAX partials) by slice workgroups of the same launch
//                     (heavy_slices).  Raw XYZZ bucket sums when level 0 runs in lanes.
//   6. bucket reduction sum_d d*B_d per window as a recursive running sum: level l splits its
//                     inputs in segments of 2^s; each segment's chain walks R += V_t, S += R,
//                     S += U_t and outputs U' = S and V' = 2^s R, so every level's outputs carry
//                     weight 1 and the last level's output IS the window sum (no scalar
//                     multiplications, no per-level tree sums, no window Horner).  Which kernel
//                     runs which level, and the record formats between them, is plan data
//                     (MsmPlan::launch, RedKernel; decided once by plan_levels, msm_common.hip):
//                     msm_device launches it and msm_scratch sizes its buffers from it.
//   7. k_final        fold over windows: sum_w 2^(c w) G_w; k_final_icicle adds ICICLE's
//                     (x, y, 1) normalisation in the same launch.
// Precompute factor F (bases table = F blocks of n bases, block f = 2^(c*Wg*f) * P) folds
// the W windows into Wg = ceil(W/F) groups so the final fold shrinks to (Wg-1)*c doublings.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "mbls_common.hpp"
#include "mbls_curve.hpp"
#include "mbls_fq28.hpp"
#include "mbls_fq2_28.hpp"
#include "mbls_rowfield.hpp"
#include "mbls_wavepoint.hpp"

namespace mbls {

static constexpr uint32_t INVALID_KEY = 0xffffffffu;

// Wave priority of the latency-bound tail kernels (bucket sums, reduction, folds).  With window
// groups they run beside the next group's VALU-saturating accumulation, and the VALU issue
// arbiter picks by priority, then age (MI355X_MICROARCH.md): raised, their chains keep issuing.
#ifndef MBLS_SETPRIO
#define MBLS_SETPRIO 3
#endif
#define MBLS_TAIL_PRIO() __builtin_amdgcn_s_setprio(MBLS_SETPRIO)
#ifndef MBLS_LIGHT_PRIO
#define MBLS_LIGHT_PRIO 2
#endif
#ifndef MBLS_CHUNK
#define MBLS_CHUNK 16
#endif
static constexpr int CHUNK = MBLS_CHUNK;  // max points per accumulation thread
static constexpr int SEG_LOG = 3;   // row segment length 8, levels >= 1 (reduction 0.96 -> 0.92 ms against 16 at G1 2^20)
static constexpr int SEG0_LOG = 2;  // level 0 (one segment per lane): short chains, many lanes
static constexpr int MAX_MSM_LOG = 26;
static constexpr int SCAN_BLOCK = 1024;
static constexpr int MAX_LEVELS = 16;

static constexpr int MAX_PRECOMPUTE = 64;
static constexpr int SMALL_MAX = 16;  // buckets of <= SMALL_MAX chunks: one thread (k_bucket_small)
static constexpr int ORDER_BINS = SMALL_MAX + 1;  // k_bucket_order bins: chunk counts 0..SMALL_MAX

// words a kernel clears in passing (grid-stride), instead of a hipMemsetAsync fill launch
struct ZeroList {
    uint32_t* p[3] = {nullptr, nullptr, nullptr};
    uint32_t n[3] = {0, 0, 0};
    MBLS_DEV void run(uint32_t gid, uint32_t stride) const {
        for (int k = 0; k < 3; ++k)
            for (uint32_t i = gid; i < n[k]; i += stride) p[k][i] = 0;
    }
};

// digit-source index of stream j of point i: j * sj + i * si (blocked: sj = n, si = 1; prepared
// point-major table: sj = 1, si = split)
struct SplitLayout {
    uint32_t sj, si;
    MBLS_DEV uint32_t at(uint32_t j, uint32_t i) const { return j * sj + i * si; }
};

// execution modes of the serial phases: one point chain per LANE (scalar arithmetic), per
// 16-lane ROW (row-sliced), or per WAVE (row-sliced, independent products spread over rows)
enum : int { MODE_LANE = 0, MODE_ROW = 1, MODE_WAVE = 2 };

// The bucket reduction's schedule (section 6), decided by plan_levels (msm_common.hip) and only
// read everywhere else: msm_device launches it, msm_scratch sizes its buffers, mbls_msm_reduce_plan
// exports it.
enum RedKernel : uint8_t {
    RED_CHAIN = 0,  // k_reduce_scaled<F, MODE>: the generic chain over Jacobian records, in the level's mode
    RED_TREE4 = 1,  // k_reduce_tree4<F>: a narrow wave level of 4-input segments
    RED_R28X = 2,   // k_reduce_scaled_r28x (G1): lane level 0 over raw XYZZ buckets
    RED_TREE8 = 3,  // k_reduce_tree8_r28x (G1): that level and the row level 1 behind it, one launch
    RED_R28PX = 4,  // k_reduce_scaled_r28px (G2): a lane level over raw pair XYZZ records
};
struct RedLaunch {
    uint8_t kernel;  // RedKernel
    uint8_t level;   // its first level
    uint8_t nlevels; // levels it covers (2: RED_TREE8)
};

struct MsmPlan {
    int c, W, Wg, F;
    int sF;                     // precomputed-table block shift in bits (0: F == 1), see window_span
    int split;                  // endomorphism split: 1 none, 2 G1 GLV (phi), 4 G2 psi
    bool prepared;              // the bases buffer is the point-major image table (no per-call table)
    int table;                  // bases-buffer entries per point (F, or split when prepared)
    int bstride;                // > 1: GLV plan on slot 0 of an F-entry shift table (make_plan)
    bool fq2;                   // G2 (Fq2 coordinates)
    uint32_t B, TB;
    uint32_t chunk;             // contributions per accumulation thread (accumulate_chunk)
    size_t pts;                 // distinct point indices (n, n*F, or split*n)
    size_t contributions;
    int levels;                 // bucket-reduction levels
    uint32_t level_m[MAX_LEVELS];  // inputs per window at each level
    uint32_t level_out[MAX_LEVELS];  // outputs per window (segments) at each level
    uint8_t seg_log[MAX_LEVELS];   // log2 segment length per level
    uint8_t mode[MAX_LEVELS];      // MODE_LANE / MODE_ROW / MODE_WAVE per level
    uint8_t off[MAX_LEVELS];       // weight of a level's input t is t + off (1 at level 0: bucket t holds digit t + 1)
    uint8_t raw_in[MAX_LEVELS];    // the level reads raw XYZZ limbs (else Jacobian words)
    uint8_t raw_out[MAX_LEVELS];   // the level writes raw XYZZ limbs
    uint8_t launch_of[MAX_LEVELS]; // the launch a level belongs to
    int launches;
    RedLaunch launch[MAX_LEVELS];
    bool bucket_raw;               // the bucket sums are raw XYZZ records (= raw_in[0])
    size_t bucket_bytes;           // a bucket record's bytes
    size_t level_bytes;            // a level output record's bytes (raw when any level writes raw)
};

// endo: the split the group offers (1 none, 2 G1 GLV, 4 G2 psi); make_plan decides whether to use it
eIcicleError make_plan(long long n, const MSMConfig* cfg, MsmPlan& p, int endo = 1);
eIcicleError plan_levels(MsmPlan& p, int Wl);
// bits between consecutive multiples in a precomputed table: [P, 2^s P, 2^(2s) P, ...], s = ceil(256 / F)
int precompute_shift(int F);

// ---- the front and the other non-templated stages (msm_common.hip) -------------------
// heavy buckets (> SMALL_MAX chunk partials), listed by k_chunk_owner for k_bucket_small's slice
// workgroups.  cnt[0] = heavy buckets, cnt[1] = slices: words TB + 1, TB + 2 of the chunk-count
// array, zeroed by the digit pass with the chunk-count maximum at TB.
struct HeavyTab {
    uint32_t* cnt;
    uint32_t* bucket;   // entry e -> its bucket
    uint32_t* first;    // entry e -> its first slice
    uint32_t* nslices;  // entry e -> its slice count
    uint32_t* done;     // entry e -> slices finished (last-block-done counter)
    uint32_t* owner;    // slice g -> its entry
    uint8_t* res;       // slice g -> its sum (Jacobian)
    uint32_t* gdone;    // planned slices: group of HEAVY_GROUP slices led by g -> slices finished
};
static constexpr uint32_t HEAVY_GDONE = 2048;  // gdone words (zeroed by k_chunk_owner)
// helpers of heavy parts (skewed scalars; msm_common.hip k_part_heavy_count): help[M] per part
// (first helper << 16 | helpers, 0: light), hh[PH_HELPERS][128] the helpers' fine counts,
// hpart[PH_HELPERS] each helper's part (~0: idle)
static constexpr uint32_t PH_HELPERS = 512;
struct PartHelp {
    uint32_t* help = nullptr;
    uint32_t* hh = nullptr;
    uint32_t* hpart = nullptr;
};
// the scratch blocks of one MSM, in arena order; msm_scratch below is their one description
struct MsmScratch {
    uint32_t *keys, *vals, *ranks;  // atomic-rank sort, c > 16 (zero bytes with the partitioned sort)
    uint8_t* dsrc;
    uint32_t *sorted, *counts, *offsets, *nchunks, *chunk_off, *tmp, *owner, *first;
    uint8_t *partials, *buckets, *levelT, *levelR, *windows;
    uint8_t* phi;                                  // the per-call image table, or null
    uint32_t *ent, *seg_off, *seg_cnt, *part_tot;  // partitioned sort (zero bytes with the atomic-rank sort)
    PartHelp ph;
    uint32_t *binhist, *binbase, *perm;  // k_bucket_order: bin histograms, their scan, bucket permutation
    HeavyTab H;
};

// digits, sort and chunk tables of one MSM on `st`: writes S.sorted, S.offsets, S.chunk_off,
// S.first, S.owner, S.perm, S.binbase, S.nchunks, S.H and, for a per-call image table, S.phi
eIcicleError msm_front(const uint8_t* scalars, bool scalars_mont, const uint8_t* bases, uint32_t n,
                       const MsmPlan& P, const MsmScratch& S, hipStream_t st);
// what msm_scratch sizes the front's blocks from.  partition_sort: c <= 16 runs the partitioned
// counting sort (pass A digits -> per-segment coarse parts, pass B per-part LDS counting sort;
// msm_common.hip 2b) instead of keys / vals / ranks + k_scatter
struct PartSortSizes {
    uint32_t NP = 0, tiles = 0, segments = 0;
    int FB = 0;
    bool pack = false;
    size_t ent = 0, segtab = 0, parts = 0;  // bytes
};
bool partition_sort(const MsmPlan& P);
PartSortSizes part_sort_sizes(const MsmPlan& P);
size_t digits_src_bytes(uint32_t n, int split);
size_t scan_tmp_words(uint32_t m);
uint32_t order_words(uint32_t m);
eIcicleError launch_scalars_from_mont(uint8_t* s, size_t n, hipStream_t st);
// host (pinned: a PCIe-reading copy kernel; pageable: hipMemcpyAsync) or peer memory -> device
eIcicleError stage_to_device(void* dst, const void* src, size_t bytes, hipStream_t st);
// point-major endomorphism image table (prepared bases): out[S i + j] = endo^j(P_i), S = 2 (G1) / 4 (G2)
eIcicleError launch_endo_table(const uint8_t* in, uint8_t* out, uint32_t n, int split, hipStream_t st);

// ------------------------------------------------------------------------------------
// 4. accumulation: thread t sums the L contributions at sorted positions [L t, L t + L),
//    one partial per bucket segment it touches (see k_chunk_counts): no idle lanes on the
//    short last chunk of each bucket.  L = accumulate_chunk: max(16, contributions per bucket
//    / 8) -- 16 at 2^20 (one 64-byte line of sorted indices per thread, ~5 partials per
//    bucket), growing with the buckets at 2^22+ so they stay off the heavy-bucket passes
//    (MBLS_ACC_CHUNK=auto: one round of resident waves, measured slower at 2^20).
//    G1 (k_accumulate_r28) works in unsaturated radix 2^28 (mbls_fq28.hpp; round 5): the lane
//    arithmetic runs on 14 x 28-bit limbs, where a column of a product is one v_mad_u64_u32 chain
//    with no carry tracking (the 32-bit FIPS product pays a v_addc per mad, and on gfx950 every
//    VALU instruction costs the same ~4 cycles: tools/valu_ceiling.hip).  Points are unpacked 8
//    bits low (x R 2^8 = x R', free).  The chunk's first point is free, its second an affine +
//    affine addition (xmmadd), and the next point is staged in LDS by LDS-DMA.  The radix-2^28
//    field values equal the word arithmetic's (tools/fq28_bench.hip; the GPU parity suite).
// ------------------------------------------------------------------------------------
// a chunk partial's bytes: the accumulator's raw radix-2^28 XYZZ limbs (4 x 14 words, per Fq2
// component for G2): no to_words conversion at the flush, which is divergent -- a bucket boundary
// falls inside ~25% of the chunks, at a different step in every lane -- and no unpack_shift8 when
// the bucket sums read them.
// With a lane-mode level 0 (every large MSM) k_bucket_small stores the bucket sums as raw XYZZ
// limbs too (store_xyzz28 / store_xyzz28p) and level 0 adds them in XYZZ (k_reduce_scaled_r28x /
// _r28px): no x_to_jac per bucket, add-2008-s instead of add-2007-bl in the level's chains, no
// unpack_shift8 on its loads
template <class F>
constexpr size_t xyzz_bytes() {  // a raw XYZZ record: chunk partial, bucket sum, G2 lane-level output
    return std::is_same<F, Fq>::value ? 224 : 448;
}
MBLS_DEV void store_xyzz28(uint8_t* __restrict__ partials, uint32_t seg, const r28::X28& acc) {
    // x, y folded (normalised, < 3p), zz, zzz normalised: valid xadd operands as they are; the
    // identity is stored as zz = 0 (the reader's test)
    uint4* q = reinterpret_cast<uint4*>(partials + (size_t)seg * 224);
    uint32_t w[56];
#pragma unroll
    for (int i = 0; i < 14; ++i) {
        w[i] = acc.x.l[i];
        w[14 + i] = acc.y.l[i];
        w[28 + i] = acc.zz.l[i];
        w[42 + i] = acc.zzz.l[i];
    }
#pragma unroll
    for (int j = 0; j < 14; ++j) q[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}
MBLS_DEV void store_jac28(uint8_t* __restrict__ partials, uint32_t seg, const r28::J28& acc) {
    Jacobian<Fq> out;
    if (acc.is_inf()) {
        out = Jacobian<Fq>::inf();
    } else {
        r28::to_words(acc.x, out.x.v);
        r28::to_words(acc.y, out.y.v);
        r28::to_words(acc.z, out.z.v);
    }
    store_jac<Fq>(partials, seg, out);
}

#ifndef MBLS_ACC_R28_MINW
#define MBLS_ACC_R28_MINW 3  // waves per SIMD the register budget is sized for (variant builds: 2)
#endif
template <class F>  // F = Fq only (a template so only msm_g1.hip instantiates it)
__global__ __launch_bounds__(256, MBLS_ACC_R28_MINW) void k_accumulate_r28(const uint32_t* __restrict__ sorted,
                                                           const uint32_t* __restrict__ offsets,
                                                           const uint32_t* __restrict__ chunk_off,
                                                           const uint32_t* __restrict__ first, uint32_t b0, uint32_t b1,
                                                           const uint8_t* __restrict__ bases,
                                                           const uint8_t* __restrict__ phi, uint32_t nsplit,
                                                           uint32_t chunk, uint8_t* __restrict__ partials) {
    const uint32_t gb = offsets[b0], ge = offsets[b1];
    const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) + gb / chunk;  // chunk index
    uint32_t beg = t * chunk;
    const uint32_t end = min(beg + chunk, ge);
    beg = max(beg, gb);
    if (beg >= end) return;
    uint32_t b = first[t];
    while (offsets[b + 1] <= beg) ++b;
    uint32_t seg = chunk_off[b] + (t - offsets[b] / chunk);
    uint32_t bend = offsets[b + 1];
    using Acc = r28::X28;
    Acc acc = Acc::inf();
    auto flush = [&](uint32_t sg) __attribute__((always_inline)) { store_xyzz28(partials, sg, acc); };
    __shared__ uint4 stage[2][256 / 64][6][64];
    // acc.y parked in the lane's half of the stage that the current point was just read from
    // (free until the next step's DMA), across the mixed addition's middle: 14 VGPRs fewer at
    // the register bound, where the compiler otherwise spilled ~30 VGPRs to scratch
    struct ParkStage {
        uint4* q;  // this lane's 6 pieces of the free slot: stage[slot][wv][k][ln], stride 64
        r28::F28 x;
        MBLS_DEV void put(int s, const r28::F28& a) {
            if (s == 0) {
                x = a;
                return;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                q[64 * k] = make_uint4(a.l[4 * k], a.l[4 * k + 1], k < 3 ? a.l[4 * k + 2] : 0u, k < 3 ? a.l[4 * k + 3] : 0u);
            asm volatile("" ::: "memory");  // the register copy is dead: reload from LDS
        }
        MBLS_DEV r28::F28 get(int s) const {
            if (s == 0) return x;
            asm volatile("" ::: "memory");
            r28::F28 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint4 u = q[64 * k];
                r.l[4 * k] = u.x;
                r.l[4 * k + 1] = u.y;
                if (k < 3) {
                    r.l[4 * k + 2] = u.z;
                    r.l[4 * k + 3] = u.w;
                }
            }
            return r;
        }
    };
    const uint32_t wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    auto issue = [&](uint32_t vv, uint32_t slot) {
        uint32_t idx = vv >> 1;
        const uint8_t* src = idx >= nsplit ? phi : bases;
        idx = idx >= nsplit ? idx - nsplit : idx;
        const uint8_t* g = src + (size_t)idx * 96;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) const void*)(g + 16 * k),
                                             (__attribute__((address_space(3))) void*)&stage[slot][wv][k][0], 16, 0, 0);
    };
    uint32_t v = sorted[beg];
    issue(v, 0);
    uint32_t vn = beg + 1 < end ? sorted[beg + 1] : v;
    for (uint32_t e = beg; e < end; ++e) {
        const uint32_t slot = (e - beg) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this point's pieces have landed
        uint32_t xw[12], yw[12], any = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint4 xa = stage[slot][wv][k][ln], ya = stage[slot][wv][3 + k][ln];
            xw[4 * k] = xa.x, xw[4 * k + 1] = xa.y, xw[4 * k + 2] = xa.z, xw[4 * k + 3] = xa.w;
            yw[4 * k] = ya.x, yw[4 * k + 1] = ya.y, yw[4 * k + 2] = ya.z, yw[4 * k + 3] = ya.w;
            any |= xa.x | xa.y | xa.z | xa.w | ya.x | ya.y | ya.z | ya.w;
        }
        if (e + 1 < end) issue(vn, slot ^ 1u);  // the other slot was read one addition ago
        const uint32_t vnn = e + 2 < end ? sorted[e + 2] : vn;
        if (e == bend) {  // bucket boundary inside the chunk: flush, move to the next bucket
            flush(seg);
            acc = Acc::inf();
            do {
                ++b;
            } while (offsets[b + 1] == e);
            seg = chunk_off[b];
            bend = offsets[b + 1];
        }
        if (any) {  // the affine identity (0, 0) adds nothing
            const r28::F28 qx = r28::unpack_shift8(xw);
            r28::F28 qy = r28::unpack_shift8(yw);
            if (v & 1) qy = r28::neg<r28::B512>(qy);  // -P: < 512 p, limbs < 2^30.4 (mbls_fq28.hpp)
            bool done = false;
            ParkStage pk{&stage[slot][wv][0][ln]};
            if (e == beg + 1 && !acc.is_inf()) done = r28::xmmadd(acc, qx, qy);
            if (!done) r28::xmadd(acc, qx, qy, pk);
        }
        v = vn;
        vn = vnn;
    }
    flush(seg);
}

// ------------------------------------------------------------------------------------
// 4'. G2 accumulation in pair-sliced radix 2^28 XYZZ (mbls_fq2_28.hpp; round 6).  The G1
//     kernel's schedule over PAIRS of lanes (lane j: component j of every Fq2 value), with the
//     next point prefetched into registers one addition ahead, the chunk's first point free and
//     its second by xmmadd; each lane's Fq2 product is one radix-2^28 product sum (no carry
//     tracking).  Equal or opposite points (H = 0) are handled inside xmadd (xdbl / identity).
// ------------------------------------------------------------------------------------
#ifndef MBLS_ACC_G2_MINW
#define MBLS_ACC_G2_MINW 2  // waves per SIMD the register budget is sized for
#endif
// G2 XYZZ partial k: lane j (component j) holds its 4 x 14 raw limbs at k * 448 + j * 224
MBLS_DEV void store_xyzz28p(uint8_t* __restrict__ partials, uint32_t seg, const r28p::X28p& acc) {
    uint4* q = reinterpret_cast<uint4*>(partials + (size_t)seg * 448 + (pairdpp::odd() ? 224 : 0));
    uint32_t w[56];
#pragma unroll
    for (int i = 0; i < 14; ++i) {
        w[i] = acc.x.l[i];
        w[14 + i] = acc.y.l[i];
        w[28 + i] = acc.zz.l[i];
        w[42 + i] = acc.zzz.l[i];
    }
#pragma unroll
    for (int j = 0; j < 14; ++j) q[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}
MBLS_DEV void xadd_raw(r28p::X28p& acc, const uint32_t (&w)[56]) {
    r28::F28 x, y, zz, zzz;
    uint32_t zany = 0;
#pragma unroll
    for (int i = 0; i < 14; ++i) {
        x.l[i] = w[i];
        y.l[i] = w[14 + i];
        zz.l[i] = w[28 + i];
        zzz.l[i] = w[42 + i];
        zany |= w[28 + i];
    }
    if (!r28p::both(zany == 0)) r28p::xadd(acc, x, y, zz, zzz);
}
// pair XYZZ sum -> the library's Jacobian words of this lane's component
MBLS_DEV Jacobian<PFq2> xyzz28p_to_words(const r28p::X28p& acc) {
    const r28p::J28p j = r28p::x_to_jac(acc);
    if (j.is_inf()) return Jacobian<PFq2>::inf();
    return {r28p::to_pf(j.x), r28p::to_pf(j.y), r28p::to_pf(j.z)};
}

template <class F>  // F = Fq2 only (a template so only msm_g2.hip instantiates it)
__global__ __launch_bounds__(256, MBLS_ACC_G2_MINW) void k_accumulate_r28p(const uint32_t* __restrict__ sorted,
                                                            const uint32_t* __restrict__ offsets,
                                                            const uint32_t* __restrict__ chunk_off,
                                                            const uint32_t* __restrict__ first, uint32_t b0,
                                                            uint32_t b1, const uint8_t* __restrict__ bases,
                                                            const uint8_t* __restrict__ phi, uint32_t nsplit,
                                                            uint32_t chunk, uint8_t* __restrict__ partials) {
    const uint32_t gb = offsets[b0], ge = offsets[b1];
    const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) / 2 + gb / chunk;  // chunk index (pair)
    uint32_t beg = t * chunk;
    const uint32_t end = min(beg + chunk, ge);
    beg = max(beg, gb);
    if (beg >= end) return;  // pair-uniform: both lanes share t
    uint32_t b = first[t];
    while (offsets[b + 1] <= beg) ++b;
    uint32_t seg = chunk_off[b] + (t - offsets[b] / chunk);
    uint32_t bend = offsets[b + 1];
    using Acc = r28p::X28p;
    Acc acc = Acc::inf();
    auto flush = [&](uint32_t sg) __attribute__((always_inline)) { store_xyzz28p(partials, sg, acc); };
    auto fetch = [&](uint32_t vv) {
        uint32_t idx = vv >> 1;
        const uint8_t* src = idx >= nsplit ? phi : bases;
        idx = idx >= nsplit ? idx - nsplit : idx;
        return load_affine<PFq2>(src, idx);  // this lane's component of x and y
    };
    uint32_t v = sorted[beg];
    Affine<PFq2> p = fetch(v);
    for (uint32_t e = beg; e < end; ++e) {
        const uint32_t vn = e + 1 < end ? sorted[e + 1] : v;
        const Affine<PFq2> pn = fetch(vn);  // one point ahead: the gather overlaps this addition
        if (e == bend) {  // bucket boundary inside the chunk: flush, move to the next bucket
            flush(seg);
            acc = Acc::inf();
            do {
                ++b;
            } while (offsets[b + 1] == e);
            seg = chunk_off[b];
            bend = offsets[b + 1];
        }
        if (!p.is_inf()) {  // the affine identity (0, 0) adds nothing (pair-uniform predicate)
            const r28::F28 qx = r28::unpack_shift8(p.x.v.v);
            r28::F28 qy = r28::unpack_shift8(p.y.v.v);
            if (v & 1) qy = r28::carry(r28::neg<r28::B512>(qy));  // -P, normalised (mbls_fq2_28.hpp)
            bool done = false;
            if (e == beg + 1 && !acc.is_inf()) done = r28p::xmmadd(acc, qx, qy);
            if (!done) r28p::xmadd(acc, qx, qy);  // equal / opposite points: xdbl / identity inside
        }
        v = vn;
        p = pn;
    }
    flush(seg);
}

// ------------------------------------------------------------------------------------
// Serial phases run on ROW-SLICED arithmetic (mbls_rowfield.hpp): one logical thread =
// one 16-lane row holding a field element limb-per-lane, so a serial chain of additions
// costs ~150 instead of ~1.3 K dependent instructions per product.  `rid` = row index.
// ------------------------------------------------------------------------------------
template <class F>
using RJac = Jacobian<typename RowOf<F>::type>;

template <class F>
MBLS_DEV RJac<F> rload_jac(const uint8_t* base, size_t idx) {
    using RO = RowOf<F>;
    const size_t q = idx * 3 * RO::FQS;
    return {RO::ld(base, q), RO::ld(base, q + RO::FQS), RO::ld(base, q + 2 * RO::FQS)};
}
template <class F>
MBLS_DEV void rstore_jac(uint8_t* base, size_t idx, const RJac<F>& a) {
    using RO = RowOf<F>;
    const size_t q = idx * 3 * RO::FQS;
    RO::st(base, q, a.x);
    RO::st(base, q + RO::FQS, a.y);
    RO::st(base, q + 2 * RO::FQS, a.z);
}
MBLS_DEV uint32_t row_id() { return (blockIdx.x * blockDim.x + threadIdx.x) >> 4; }

// ------------------------------------------------------------------------------------
// 6. one level of the recursive running-sum reduction.
//   in:  V[w * m_in + k], k < m_in, weight (k + off)
//   out: T[w * m_out + q], R[w * m_out + q], m_out = ceil(m_in / seg)
// Level 0 has plenty of segments and runs one segment per LANE (scalar arithmetic, short
// segments); the later, narrower levels run one segment per ROW (row-sliced arithmetic).
// Single jac_add call site: the loop alternates the R and S updates.
// ------------------------------------------------------------------------------------
// the execution modes (MODE_LANE / MODE_ROW / MODE_WAVE, above MsmPlan) as point arithmetic
template <class F, int MODE>
struct RedIO;
template <class F>
struct RedIO<F, MODE_LANE> {
    using L = typename LaneOf<F>::type;
    using J = Jacobian<L>;
    MBLS_DEV static uint32_t id() { return (blockIdx.x * blockDim.x + threadIdx.x) / LaneOf<F>::LANES; }
    MBLS_DEV static J ld(const uint8_t* b, size_t i) { return load_jac<L>(b, i); }
    MBLS_DEV static void st(uint8_t* b, size_t i, const J& v) { store_jac<L>(b, i, v); }
    MBLS_DEV static J add(const J& a, const J& b) { return jac_add(a, b); }
    MBLS_DEV static J dbl(const J& a) { return jac_dbl(a); }
};
template <class F>
struct RedIO<F, MODE_ROW> {
    using J = RJac<F>;
    MBLS_DEV static uint32_t id() { return row_id(); }
    MBLS_DEV static J ld(const uint8_t* b, size_t i) { return rload_jac<F>(b, i); }
    MBLS_DEV static void st(uint8_t* b, size_t i, const J& v) { rstore_jac<F>(b, i, v); }
    MBLS_DEV static J add(const J& a, const J& b) { return jac_add(a, b); }
    MBLS_DEV static J dbl(const J& a) { return jac_dbl(a); }
};
template <class F>
struct RedIO<F, MODE_WAVE> {
    using J = RJac<F>;
    MBLS_DEV static uint32_t id() { return (blockIdx.x * blockDim.x + threadIdx.x) >> 6; }
    MBLS_DEV static J ld(const uint8_t* b, size_t i) { return rload_jac<F>(b, i); }
    MBLS_DEV static void st(uint8_t* b, size_t i, const J& v) {
        if (wave::leader_row()) rstore_jac<F>(b, i, v);
    }
    MBLS_DEV static J add(const J& a, const J& b) { return wave::jadd(a, b); }
    MBLS_DEV static J dbl(const J& a) { return wave::jdbl(a); }
};
template <int MODE>
constexpr uint32_t lanes_per_chain() { return MODE == MODE_LANE ? 1u : MODE == MODE_ROW ? 16u : 64u; }

// ------------------------------------------------------------------------------------
// 5. bucket sums from chunk partials.  Light buckets (<= SMALL_MAX partials -- every bucket of
//    random inputs): one thread each.  Heavy buckets (equal scalars, adversarial inputs): cut into
//    slices (heavy_slices' plan, or HEAVY_SLICE partials listed by k_chunk_owner); one workgroup per slice
//    sums its slice (strided chains + an LDS tree), and the workgroup that finishes a bucket's
//    last slice (a counter per bucket: last-block-done) sums the bucket's slice sums.  The slice
//    workgroups ride in the same launch as the light buckets (HEAVY_BLOCKS extra workgroups that
//    exit at once when there is no heavy bucket): no extra launch, no side stream, no event.
// ------------------------------------------------------------------------------------
#ifndef MBLS_HEAVY_SLICE
#define MBLS_HEAVY_SLICE 2048
#endif
static constexpr uint32_t HEAVY_SLICE = MBLS_HEAVY_SLICE;  // chunk partials per heavy slice (one workgroup)
static constexpr uint32_t HEAVY_BLOCKS = 512;  // workgroups appended to k_bucket_small (two per CU)

// Heavy buckets: a slice workgroup's lanes sum strided chains of its partials (lane arithmetic:
// throughput), then its 16 rows sum the chain results ROW-SLICED (RedIO<MODE_ROW>: one 16-lane
// row per chain, ~5 us per Jacobian addition against ~25 us for a lone lane at one wave per SIMD)
// and a 4-level row tree through LDS finishes; the slice sums of a bucket are added the same way
// by the workgroup that finishes its last slice.  The former 8-level lane tree per slice took
// 0.58 ms for one bucket of 2^16 partials (G1 2^20, every scalar 1) and 1.44 ms for 16.
template <class F>
MBLS_DEV RJac<F> row_tree(RJac<F> acc, uint8_t* sh, uint32_t r) {
    using IO = RedIO<F, MODE_ROW>;
    constexpr uint32_t ROWS = 256 / 16;
    IO::st(sh, r, acc);
    __syncthreads();
    for (uint32_t s = ROWS / 2; s > 0; s >>= 1) {
        if (r < s) {
            acc = IO::add(acc, IO::ld(sh, r + s));
            IO::st(sh, r, acc);
        }
        __syncthreads();
    }
    return acc;
}

// sum of n <= 16 Jacobian points ld(k) by the workgroup's 4 waves in the wave layout (a wave
// addition spreads its independent products over the 4 rows: ~1/3 of a row addition's latency):
// wave w adds points w, w + 4, ... (<= 3 additions), wave 0 adds the 3 other wave sums through
// sh slots 1..3 (a wave writes only its own slot, read by no other wave before the barrier).
// Result valid in wave 0.  6 dependent additions against the row tree's 4 x ~3.
template <class F, class Ld>
MBLS_DEV RJac<F> wave_sum16(uint8_t* sh, uint32_t n, Ld&& ld) {
    using W = RedIO<F, MODE_WAVE>;
    const uint32_t wv = threadIdx.x >> 6;
    RJac<F> acc = wv < n ? ld(wv) : RJac<F>::inf();
    for (uint32_t k = wv + 4; k < n; k += 4) acc = W::add(acc, ld(k));
    W::st(sh, wv, acc);
    __syncthreads();
    if (wv == 0)
        for (uint32_t k = 1; k < 4 && k < n; ++k) acc = W::add(acc, W::ld(sh, k));
    __syncthreads();  // sh is reused by the caller
    return acc;
}

// sum of the CHAINS Jacobian points in sh (lane layout), by rows; result in row 0
template <class F>
MBLS_DEV RJac<F> rows_sum_chains(uint8_t* sh, uint32_t chains) {
    using IO = RedIO<F, MODE_ROW>;
    constexpr uint32_t ROWS = 256 / 16;
    const uint32_t r = threadIdx.x >> 4;
    RJac<F> acc = r < chains ? IO::ld(sh, r) : RJac<F>::inf();  // no addition to the identity first
    for (uint32_t k = r + ROWS; k < chains; k += ROWS) acc = IO::add(acc, IO::ld(sh, k));
    // row r has read its slots (k = r, r + 16, ...); row_tree overwrites only slot r < 16
    return row_tree<F>(acc, sh, r);
}

// inclusive wave64 scan (shuffles)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

MBLS_DEV bool load_j28(const uint8_t* __restrict__ base, size_t i, r28::F28& x, r28::F28& y, r28::F28& z) {
    const uint4* q = reinterpret_cast<const uint4*>(base + i * 144);
    uint32_t w[3][12], zany = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint4 u = q[3 * c + j];
            w[c][4 * j] = u.x, w[c][4 * j + 1] = u.y, w[c][4 * j + 2] = u.z, w[c][4 * j + 3] = u.w;
        }
#pragma unroll
    for (int j = 0; j < 12; ++j) zany |= w[2][j];
    if (!zany) return false;  // the identity
    x = r28::unpack_shift8(w[0]);
    y = r28::unpack_shift8(w[1]);
    z = r28::unpack_shift8(w[2]);
    return true;
}
// the 56 raw words of XYZZ record k (224 B; `half` selects the odd lane's half of a 448-B pair record)
MBLS_DEV void load_raw56(const uint8_t* __restrict__ recs, size_t off, uint32_t (&w)[56]) {
    const uint4* q = reinterpret_cast<const uint4*>(recs + off);
#pragma unroll
    for (int j = 0; j < 14; ++j) {
        const uint4 u = q[j];
        w[4 * j] = u.x, w[4 * j + 1] = u.y, w[4 * j + 2] = u.z, w[4 * j + 3] = u.w;
    }
}
MBLS_DEV void xadd_raw(r28::X28& acc, const uint32_t (&w)[56]) {
    r28::F28 x, y, zz, zzz;
    uint32_t zany = 0;
#pragma unroll
    for (int i = 0; i < 14; ++i) {
        x.l[i] = w[i];
        y.l[i] = w[14 + i];
        zz.l[i] = w[28 + i];
        zzz.l[i] = w[42 + i];
        zany |= w[28 + i];
    }
    if (zany) r28::xadd(acc, x, y, zz, zzz);
}
// XYZZ addition of chunk partial k (the light path's and the slice chains' form; raw limbs,
// store_xyzz28 / store_xyzz28p); the identity (zz = 0) adds nothing
MBLS_DEV void r28_add_partial(r28::X28& acc, const uint8_t* __restrict__ partials, uint32_t k) {
    uint32_t w[56];
    load_raw56(partials, (size_t)k * 224, w);
    xadd_raw(acc, w);
}
MBLS_DEV void r28p_add_partial(r28p::X28p& acc, const uint8_t* __restrict__ partials, uint32_t k) {
    uint32_t w[56];
    load_raw56(partials, (size_t)k * 448 + (pairdpp::odd() ? 224 : 0), w);
    xadd_raw(acc, w);
}

// Slice plan (round 5): the slice length S adapts to the heavy partials T of the call, S =
// clamp(pow2 >= T / (slice workgroups), HEAVY_SLICE_MIN, HEAVY_SLICE), so that few heavy buckets
// (half the scalars 1: one bucket of 2^15 partials at G1 2^20) spread over many workgroups
// instead of 16 slices of 8-deep lane chains, while many (one repeated scalar: 16 buckets of 2^16)
// keep 2048-partial slices, one round of workgroups.  Every slice workgroup derives the plan from
// the heavy-bucket list (their chunk counts, a prefix of slices per bucket in LDS); more than
// HEAVY_LDS heavy buckets take k_chunk_owner's fixed HEAVY_SLICE plan (H.owner / first / nslices).
// Planned slices finish in groups of HEAVY_GROUP: the workgroup finishing a group's last slice
// sums the group (one row each, a 4-level row tree), the one finishing a bucket's last group sums
// the group sums -- with 64-partial slices a bucket of 2^15 partials takes 3 + 4, 4 and 2 + 4
// dependent row additions instead of 16 + 4 and 32 + 4 in one level.
#ifndef MBLS_HEAVY_SLICE_MIN
#define MBLS_HEAVY_SLICE_MIN 256
#endif
static constexpr uint32_t HEAVY_SLICE_MIN = MBLS_HEAVY_SLICE_MIN, HEAVY_LDS = 1024, HEAVY_GROUP = 16;

// a bucket's row-layout sum (limb j on lane j of row 0 -- wave layout's leader row, or the row
// tree's row 0) into `buckets`: Jacobian words (rstore_jac), or with xb the raw XYZZ limbs of
// (X, Y, Z^2, Z^3) the lane-mode level 0 reads (k_reduce_scaled_r28x).  Wave 0, all 64 lanes.
template <class F>
MBLS_DEV void store_bucket_row(uint8_t* __restrict__ buckets, uint32_t b, const RJac<F>& p, bool xb) {
    if constexpr (std::is_same<F, Fq>::value) {
        if (xb) {
            uint32_t w[3][12], zany = 0;
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                w[0][i] = (uint32_t)__shfl((int)p.x.v, i, 64);
                w[1][i] = (uint32_t)__shfl((int)p.y.v, i, 64);
                w[2][i] = (uint32_t)__shfl((int)p.z.v, i, 64);
                zany |= w[2][i];
            }
            if (threadIdx.x != 0) return;
            r28::X28 a = r28::X28::inf();
            if (zany) {
                const r28::F28 z = r28::unpack_shift8(w[2]);
                a.x = r28::fold(r28::unpack_shift8(w[0]));
                a.y = r28::fold(r28::unpack_shift8(w[1]));
                a.zz = r28::sqr(z);
                a.zzz = r28::mul(a.zz, z);
            }
            store_xyzz28(buckets, b, a);
            return;
        }
    }
    if constexpr (std::is_same<F, Fq2>::value) {
        if (xb) {  // every lane of wave 0 forms its pair component (c0 on even lanes, c1 on odd)
            const bool odd = pairdpp::odd();
            uint32_t w[3][12], zany = 0;
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                const uint32_t x0 = (uint32_t)__shfl((int)p.x.c0.v, i, 64), x1 = (uint32_t)__shfl((int)p.x.c1.v, i, 64);
                const uint32_t y0 = (uint32_t)__shfl((int)p.y.c0.v, i, 64), y1 = (uint32_t)__shfl((int)p.y.c1.v, i, 64);
                const uint32_t z0 = (uint32_t)__shfl((int)p.z.c0.v, i, 64), z1 = (uint32_t)__shfl((int)p.z.c1.v, i, 64);
                w[0][i] = odd ? x1 : x0;
                w[1][i] = odd ? y1 : y0;
                w[2][i] = odd ? z1 : z0;
                zany |= z0 | z1;
            }
            r28p::X28p a = r28p::X28p::inf();
            if (zany) {  // wave-uniform
                const r28::F28 z = r28::fold(r28::unpack_shift8(w[2]));
                a.x = r28::fold(r28::unpack_shift8(w[0]));
                a.y = r28::fold(r28::unpack_shift8(w[1]));
                a.zz = r28p::sqr<r28::B16>(z);
                a.zzz = r28p::mul<r28::B16>(a.zz, z);
            }
            if (threadIdx.x < 2) store_xyzz28p(buckets, b, a);
            return;
        }
    }
    if (wave::leader_row()) rstore_jac<F>(buckets, b, p);
}

template <class F>
MBLS_DEV void heavy_slices(const uint32_t* __restrict__ chunk_off, const uint8_t* __restrict__ partials,
                           uint8_t* __restrict__ buckets, const HeavyTab& H, uint32_t hb, uint32_t nhb, bool xb) {
    using L = typename LaneOf<F>::type;
    using IO = RedIO<F, MODE_ROW>;
    constexpr uint32_t LN = LaneOf<F>::LANES;
    constexpr uint32_t CHAINS = 256 / LN;
    __shared__ __attribute__((aligned(16))) uint8_t sh[CHAINS * 3 * sizeof(F)];
    __shared__ uint32_t last, hfirst[HEAVY_LDS + 1], wred[4];
    const uint32_t nh = H.cnt[0];
    if (nh == 0) return;  // workgroup-uniform (random scalars: every slice workgroup leaves here)
    const bool planned = nh <= HEAVY_LDS;
    uint32_t S = HEAVY_SLICE, nsl = H.cnt[1];
    if (planned) {
        const uint32_t per = (nh + 255) / 256, e0 = min(threadIdx.x * per, nh), e1 = min(e0 + per, nh);
        uint32_t t = 0;
        for (uint32_t e = e0; e < e1; ++e) {
            const uint32_t b = H.bucket[e];
            t += chunk_off[b + 1] - chunk_off[b];
        }
        uint32_t r = t;
        for (int d = 32; d > 0; d >>= 1) r += __shfl_xor(r, d, 64);
        if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = r;
        __syncthreads();
        const uint32_t T = wred[0] + wred[1] + wred[2] + wred[3];
        const uint32_t want = (T + nhb - 1) / nhb;
        S = HEAVY_SLICE_MIN;
        while (S < want && S < HEAVY_SLICE) S <<= 1;
        uint32_t c = 0;
        for (uint32_t e = e0; e < e1; ++e) {
            const uint32_t b = H.bucket[e];
            c += (chunk_off[b + 1] - chunk_off[b] + S - 1) / S;
        }
        const uint32_t incl = wave_incl_scan(c);
        __syncthreads();  // wred is reused
        if ((threadIdx.x & 63) == 63) wred[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t f = incl - c;
        for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k) f += wred[k];
        for (uint32_t e = e0; e < e1; ++e) {
            const uint32_t b = H.bucket[e];
            hfirst[e] = f;
            f += (chunk_off[b + 1] - chunk_off[b] + S - 1) / S;
        }
        if (e1 == nh && e0 < e1) hfirst[nh] = f;
        __syncthreads();
        nsl = hfirst[nh];
    }
    // slices <= nhb + nh with S >= T / nhb: within HEAVY_GDONE for nh <= HEAVY_LDS (checked anyway)
    const bool grouped = planned && nsl <= HEAVY_GDONE;
    const uint32_t j = threadIdx.x / LN;
    for (uint32_t g = hb; g < nsl; g += nhb) {
        uint32_t e, f0, ns;
        if (planned) {  // the bucket whose slices hold g: last e with hfirst[e] <= g
            uint32_t lo = 0, hi = nh;  // hfirst[lo] <= g < hfirst[hi]
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (hfirst[mid] <= g)
                    lo = mid;
                else
                    hi = mid;
            }
            e = lo, f0 = hfirst[lo], ns = hfirst[lo + 1] - f0;
        } else {
            e = H.owner[g], f0 = H.first[e], ns = H.nslices[e];
        }
        const uint32_t b = H.bucket[e];
        const uint32_t c0 = chunk_off[b] + (g - f0) * S;
        const uint32_t c1 = min(c0 + S, chunk_off[b + 1]);
        // chains, then a lane tree down to 16 chain sums (log depth: a lane addition is ~1.3x a
        // row addition's latency, but 16 rows summing 256 chains took 15 of them in series), then
        // the rows
        uint32_t live = min(CHAINS, c1 - c0);
        if constexpr (std::is_same<L, Fq>::value) {
            r28::X28 xacc = r28::X28::inf();
            for (uint32_t k = c0 + j; k < c1; k += CHAINS) r28_add_partial(xacc, partials, k);
            r28::J28 acc = r28::x_to_jac(xacc);  // the lane tree below adds Jacobian chain sums
            store_jac28(sh, j, acc);
            __syncthreads();
            for (; live > 16; live = (live + 1) / 2) {
                const uint32_t h = (live + 1) / 2;  // chain j < live - h takes chain j + h
                if (j < live - h) {
                    r28::F28 x, y, z;
                    if (load_j28(sh, j + h, x, y, z)) r28::jadd(acc, x, y, z);
                }
                __syncthreads();
                if (j < live - h) store_jac28(sh, j, acc);
                __syncthreads();
            }
        } else {
            r28p::X28p xacc = r28p::X28p::inf();
            for (uint32_t k = c0 + j; k < c1; k += CHAINS) r28p_add_partial(xacc, partials, k);
            Jacobian<L> acc = xyzz28p_to_words(xacc);  // the lane tree below adds Jacobian chain sums
            store_jac<L>(sh, j, acc);
            __syncthreads();
            for (; live > 16; live = (live + 1) / 2) {
                const uint32_t h = (live + 1) / 2;
                if (j < live - h) acc = jac_add(acc, load_jac<L>(sh, j + h));
                __syncthreads();
                if (j < live - h) store_jac<L>(sh, j, acc);
                __syncthreads();
            }
        }
        using WIO = RedIO<F, MODE_WAVE>;
        const RJac<F> ssum = wave_sum16<F>(sh, live, [&](uint32_t k) { return WIO::ld(sh, k); });
        if (threadIdx.x < 64) WIO::st(H.res, g, ssum);
        __threadfence();
        __syncthreads();
        const uint32_t r = threadIdx.x >> 4;
        // the sums to combine at the bucket level: slice sums (one level), or the group sums at
        // f0, f0 + HEAVY_GROUP, ... (grouped)
        uint32_t nsum = ns, step = 1;
        if (grouped) {
            const uint32_t gl = f0 + (g - f0) / HEAVY_GROUP * HEAVY_GROUP;  // the group's first slice
            const uint32_t gs = min(HEAVY_GROUP, f0 + ns - gl);
            if (threadIdx.x == 0) last = atomicAdd(&H.gdone[gl], 1u) + 1 == gs ? 1u : 0u;
            __syncthreads();
            if (!last) continue;  // workgroup-uniform; sh and `last` are rewritten after barriers
            __threadfence();
            const RJac<F> gsum = wave_sum16<F>(sh, gs, [&](uint32_t k) { return WIO::ld(H.res, gl + k); });
            if (threadIdx.x < 64) WIO::st(H.res, gl, gsum);
            __threadfence();
            __syncthreads();
            nsum = (ns + HEAVY_GROUP - 1) / HEAVY_GROUP, step = HEAVY_GROUP;
        }
        if (threadIdx.x == 0) last = atomicAdd(&H.done[e], 1u) + 1 == nsum ? 1u : 0u;
        __syncthreads();
        if (last) {  // this workgroup finished bucket b's last slice (group): sum the sums
            __threadfence();
            if (nsum <= 16) {  // workgroup-uniform
                const RJac<F> tot = wave_sum16<F>(sh, nsum, [&](uint32_t k) { return WIO::ld(H.res, f0 + k * step); });
                if (threadIdx.x < 64) store_bucket_row<F>(buckets, b, tot, xb);
            } else {
                RJac<F> tot = r < nsum ? IO::ld(H.res, f0 + r * step) : RJac<F>::inf();
                for (uint32_t k = r + 16; k < nsum; k += 16) tot = IO::add(tot, IO::ld(H.res, f0 + k * step));
                tot = row_tree<F>(tot, sh, r);
                if (threadIdx.x < 64) store_bucket_row<F>(buckets, b, tot, xb);
            }
        }
        __syncthreads();  // sh and `last` are reused by the next slice
    }
}

// light buckets: one thread per bucket (<= SMALL_MAX chunks) sums its chunk partials; thread t
// takes perm[start + t] (k_chunk_owner: buckets grouped by chunk count, heaviest first, so a
// wave's lanes run the same number of additions).  The first HEAVY_BLOCKS workgroups take the
// heavy slices, the light buckets' `light_blocks` follow.
template <class F>
// 2 waves per SIMD: G1 fits anyway (181 VGPRs); G2's pair-sliced sums took 260 VGPRs + 4 AGPRs,
// i.e. one latency-bound wave per SIMD -- capped at 256 (4 spilled) its bucket sums take 0.93
// instead of 1.17 ms at 2^20 (A/B x2 on one box, profiles/r04/bs_minw_ab.txt)
#ifndef MBLS_BS_MINW
#define MBLS_BS_MINW 2
#endif
__global__ __launch_bounds__(256, MBLS_BS_MINW) void k_bucket_small(const uint32_t* __restrict__ chunk_off,
                                                      const uint32_t* __restrict__ perm, const uint32_t* __restrict__ binbase,
                                                      uint32_t gwords, const uint8_t* __restrict__ partials,
                                                      uint8_t* __restrict__ buckets, uint32_t light_blocks, HeavyTab H,
                                                      int xb) {
    MBLS_TAIL_PRIO();
    using L = typename LaneOf<F>::type;
    // the slice workgroups come first: dispatched at once, the heavy buckets' chains overlap the
    // light buckets (they used to start behind them: G1 2^20 half ones ~0.1 ms)
    if (blockIdx.x < HEAVY_BLOCKS) {
        heavy_slices<F>(chunk_off, partials, buckets, H, blockIdx.x, HEAVY_BLOCKS, xb != 0);
        return;
    }
    // light workgroups one wave-priority step below the slice workgroups: the heavy buckets'
    // dependent row chains share CUs with them (G1 2^20 half ones: a bucket-level row tree took
    // 130-220 us beside light sums instead of ~45)
    __builtin_amdgcn_s_setprio(MBLS_LIGHT_PRIO);
    const uint32_t start = binbase[0], stop = binbase[gwords];
    const uint32_t t = start + ((blockIdx.x - HEAVY_BLOCKS) * blockDim.x + threadIdx.x) / LaneOf<F>::LANES;
    if (t >= stop) return;
    const uint32_t b = perm[t];
    const uint32_t k0 = chunk_off[b], k1 = chunk_off[b + 1];
    if constexpr (std::is_same<L, Fq>::value) {
        // radix 2^28: XYZZ sums of XYZZ partials (add-2008-s), one conversion per bucket (round 6)
        r28::X28 acc = r28::X28::inf();
        for (uint32_t k = k0; k < k1; ++k) r28_add_partial(acc, partials, k);
        if (xb)
            store_xyzz28(buckets, b, acc);
        else
            store_jac28(buckets, b, r28::x_to_jac(acc));
    } else {
        // pair-sliced radix-2^28 XYZZ sums of the raw XYZZ partials (round 6), one conversion
        r28p::X28p acc = r28p::X28p::inf();
        for (uint32_t k = k0; k < k1; ++k) r28p_add_partial(acc, partials, k);
        if (xb)
            store_xyzz28p(buckets, b, acc);
        else
            store_jac<L>(buckets, b, xyzz28p_to_words(acc));
    }
}

// Scaled running-sum level: every level's outputs carry weight 1, so
// the last level's single output per window IS the window sum -- no per-level T tree sums on side
// streams and no window Horner.  Level l sees inputs with
//   G_w = sum_k ((k + off) V_k + U_k)            (level 0: V = buckets, off = 1, no U)
// and segment q = [k0, k1) of 2^s inputs produces
//   U'_q = sum_t (t - k0 + off) V_t + sum_t U_t   (running sum: R += V_t; S += R; S += U_t)
//   V'_q = 2^s sum_t V_t                           (s doublings of R)
// so that G_w = sum_q (q V'_q + U'_q): the same form with off = 0.  One add call site (the three
// steps of a t alternate), one doubling call site.
template <class F, int MODE>
__global__ __launch_bounds__(256) void k_reduce_scaled(const uint8_t* __restrict__ V, const uint8_t* __restrict__ U,
                                                       uint32_t m_in, uint32_t seg_log, int Wg, int off,
                                                       uint8_t* __restrict__ Vout, uint8_t* __restrict__ Uout) {
    MBLS_TAIL_PRIO();
    using IO = RedIO<F, MODE>;
    using J = typename IO::J;
    const uint32_t seg = 1u << seg_log;
    const uint32_t m_out = (m_in + seg - 1) >> seg_log;
    const uint32_t tid = IO::id();
    if (tid >= m_out * (uint32_t)Wg) return;
    const uint32_t w = tid / m_out, q = tid % m_out;
    const uint32_t k0 = q << seg_log;
    const uint32_t k1 = min(k0 + seg, m_in);  // exclusive
    const size_t base = (size_t)w * m_in;
    J R = J::inf(), S = J::inf();
    uint32_t t = k1 - 1;
    int ph = 0;  // 0: R += V_t, 1: S += R, 2: S += U_t
    while (true) {
        const bool skip = (ph == 1 && (t - k0) + off == 0) || (ph == 2 && !U);
        if (!skip) {
            const J x = ph == 0 ? R : S;
            const J y = ph == 0 ? IO::ld(V, base + t) : ph == 1 ? R : IO::ld(U, base + t);
            const J z = IO::add(x, y);
            if (ph == 0)
                R = z;
            else
                S = z;
        }
        if (ph == 2) {
            if (t == k0) break;
            --t;
            ph = 0;
        } else {
            ++ph;
        }
    }
    if (Vout) {
        for (uint32_t k = 0; k < seg_log; ++k) R = IO::dbl(R);
        IO::st(Vout, tid, R);
    }
    IO::st(Uout, tid, S);
}

// G1's lane-mode level 0 over raw XYZZ buckets (MsmPlan::bucket_raw, no U) in radix 2^28: the chain of
// k_reduce_scaled with add-2008-s (r28::xadd, 12M + 2S) for its two additions per step, the
// outputs converted once.  Bucket t - 1 is loaded before bucket t is added.
// One lane's chain over buckets [k0, k1) of the window at record `base`: S = sum (t - k0 + off) V_t
// and, with `scale`, R = 2^seg_log sum V_t (else the plain sum).  An empty range leaves both the
// identity, and a doubled identity stays exactly zz = 0.
MBLS_DEV void r28x_chain(const uint8_t* __restrict__ V, uint32_t base, uint32_t k0, uint32_t k1, uint32_t seg_log,
                         int off, bool scale, r28::X28& R, r28::X28& S) {
    R = r28::X28::inf(), S = r28::X28::inf();
    if (k1 <= k0) return;
    uint32_t nw[56];  // bucket t - 1, loaded while bucket t is added (one wave per SIMD: nothing else hides it)
    load_raw56(V, (size_t)(base + k1 - 1) * 224, nw);
    for (uint32_t t = k1; t-- > k0;) {
        uint32_t cw[56];
#pragma unroll
        for (int i = 0; i < 56; ++i) cw[i] = nw[i];
        if (t > k0) load_raw56(V, (size_t)(base + t - 1) * 224, nw);
        xadd_raw(R, cw);                                                                   // R += V_t
        if ((t - k0) + off != 0 && !R.is_inf()) r28::xadd(S, R.x, R.y, R.zz, R.zzz);  // S += R
    }
    if (scale && !R.is_inf())
        for (uint32_t k = 0; k < seg_log; ++k) r28::xdbl(R);
}
template <class F>  // F = Fq only
__global__ __launch_bounds__(256) void k_reduce_scaled_r28x(const uint8_t* __restrict__ V, uint32_t m_in,
                                                            uint32_t seg_log, int Wg, int off,
                                                            uint8_t* __restrict__ Vout, uint8_t* __restrict__ Uout) {
    MBLS_TAIL_PRIO();
    const uint32_t seg = 1u << seg_log;
    const uint32_t m_out = (m_in + seg - 1) >> seg_log;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= m_out * (uint32_t)Wg) return;
    const uint32_t w = tid / m_out, q = tid % m_out;
    const uint32_t k0 = q << seg_log;
    const uint32_t k1 = min(k0 + seg, m_in);  // exclusive
    r28::X28 R, S;
    r28x_chain(V, w * m_in, k0, k1, seg_log, off, Vout != nullptr, R, S);
    if (Vout) store_jac28(Vout, tid, r28::x_to_jac(R));
    store_jac28(Uout, tid, r28::x_to_jac(S));
}

// G1's level 1 (row plan: segments of 8, off = 0) as a tree in lane arithmetic.  A segment's
// outputs are linear in its inputs,
//   U' = sum_j U_j + sum_j j V_j = sum U + T0 + 2 T1 + 4 T2   (T_b: the V_j with bit b of j set)
//   V' = 8 sum_j V_j,
// so eight adjacent lanes evaluate them in six passes of one r28::xadd and / or one r28::xdbl per
// lane instead of the chain's 27 dependent row-sliced operations.  Lane j enters with V_j, U_j
// (the identity past the level's end); X is its running value, operands cross lanes as the 56 raw
// limbs by ds_bpermute (no LDS, no barrier).  P_i = V_2i + V_2i+1, Q_i = U_2i + U_2i+1:
//   pass 0 add: lane 2i: P_i = V_2i + V_2i+1                lane 2i+1: Q_i = U_2i+1 + U_2i
//   pass 1 add: 0: P0 + P1   2: T1 = P1 + P3   4: T2 = P2 + P3   1: Q0 + Q1   5: Q2 + Q3
//               3: V3 + V1   7: V7 + V5
//   pass 2 add: 0: SV = (P0 + P1) + T2   2: T1 + T2   3: T0 = (V3 + V1) + (V7 + V5)   1: SU
//   pass 3 add: 2: W = (T1 + T2) + T2    1: E = SU + T0          dbl: 0: 2 SV
//   pass 4                                                       dbl: 2: 2 W    0: 4 SV
//   pass 5 add: 1: U' = E + 2 W                                  dbl: 0: V' = 8 SV
// Doublings share only passes 3 and 5 with additions (a wave holding both issues both bodies).
// Every addition is xadd with its identity / equal / opposite branches -- the tree meets operand
// coincidences the chain never did (T1 = T2, E = 2 W, V_j = +-V_k) -- and the identity is never
// doubled, so it stays exactly zz = 0 (tests/reduce_tree_model.py restates the sites).
// Lanes 0 and 1 convert once and store V', U' as the Jacobian words the wave levels read.
MBLS_DEV r28::X28 lane_fetch(const r28::X28& p, uint32_t src_byte) {
    r28::X28 r;
#pragma unroll
    for (int i = 0; i < r28::NL; ++i) {
        r.x.l[i] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src_byte, (int)p.x.l[i]);
        r.y.l[i] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src_byte, (int)p.y.l[i]);
        r.zz.l[i] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src_byte, (int)p.zz.l[i]);
        r.zzz.l[i] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src_byte, (int)p.zzz.l[i]);
    }
    return r;
}
// sel: 0 a, 1 b, 2 c
MBLS_DEV r28::X28 lane_pick(uint32_t sel, const r28::X28& a, const r28::X28& b, const r28::X28& c) {
    r28::X28 r;
#pragma unroll
    for (int i = 0; i < r28::NL; ++i) {
        r.x.l[i] = sel == 0 ? a.x.l[i] : sel == 1 ? b.x.l[i] : c.x.l[i];
        r.y.l[i] = sel == 0 ? a.y.l[i] : sel == 1 ? b.y.l[i] : c.y.l[i];
        r.zz.l[i] = sel == 0 ? a.zz.l[i] : sel == 1 ? b.zz.l[i] : c.zz.l[i];
        r.zzz.l[i] = sel == 0 ? a.zzz.l[i] : sel == 1 ? b.zzz.l[i] : c.zzz.l[i];
    }
    return r;
}
// All 64 lanes of the wave call it together (the fetches read the other lanes' registers).
// Returns lane 0's V' and lane 1's U' of each group of eight.
MBLS_DEV r28::X28 reduce_tree8(const r28::X28& V, const r28::X28& U) {
    const uint32_t lane = __lane_id(), j = lane & 7;
    r28::X28 X = r28::X28::inf();
#pragma unroll 1
    for (int p = 0; p < 6; ++p) {
        // per pass: the lanes that add / double (bit j), the lane each adding lane fetches from
        // (nibble j), what a lane fetches from holds out and what an adding lane adds to (two
        // bits per lane: 0 X, 1 V, 2 U)
        const uint32_t addm = (uint32_t)(0x0200060fbfffull >> (8 * p)) & 0xffu;
        const uint32_t dblm = (uint32_t)(0x010501000000ull >> (8 * p)) & 0xffu;
        if (addm) {  // wave-uniform
            const uint32_t src = p == 0 ? 0x67452301u : p == 1 ? 0x56761632u : p == 2 ? 0x76547454u
                                 : p == 3 ? 0x76543430u : 0x76543220u;
            const uint32_t pub = p == 0 ? 0x6666u : p == 1 ? 0x0404u : 0u;
            const uint32_t own = p == 0 ? 0x9999u : p == 1 ? 0x4040u : 0u;
            const r28::X28 out = lane_pick((pub >> (2 * j)) & 3u, X, V, U);
            X = lane_pick((own >> (2 * j)) & 3u, X, V, U);
            const r28::X28 b = lane_fetch(out, ((lane & ~7u) | ((src >> (4 * j)) & 7u)) << 2);
            if (((addm >> j) & 1u) && !b.is_inf()) r28::xadd(X, b.x, b.y, b.zz, b.zzz);
        }
        if (((dblm >> j) & 1u) && !X.is_inf()) r28::xdbl(X);
    }
    return X;
}
// Levels 0 and 1 in one launch: lane (segment, j) first runs the level-0 chain whose outputs are
// the segment's inputs j (V: the raw bucket sums, m0 per window, level-0 segments of 2^seg0_log),
// keeps them in registers and goes straight into the tree -- no hand-over through memory, one
// launch fewer (the plan still counts two levels).  m_in: level 1's inputs per window.  No lane
// returns before the tree.
template <class F>  // F = Fq only
__global__ __launch_bounds__(256) void k_reduce_tree8_r28x(const uint8_t* __restrict__ V, uint32_t m0, uint32_t seg0_log,
                                                           uint32_t m_in, int Wg, uint8_t* __restrict__ Vout,
                                                           uint8_t* __restrict__ Uout) {
    MBLS_TAIL_PRIO();
    const uint32_t m_out = (m_in + 7) >> 3;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t w = tid / (8 * m_out), q = tid % (8 * m_out);  // q: the input's index in its window
    const bool live = w < (uint32_t)Wg && q < m_in;
    r28::X28 Vj, Uj;
    const uint32_t k0 = q << seg0_log;
    const uint32_t k1 = live ? min(k0 + (1u << seg0_log), m0) : k0;  // an empty range: the identity
    r28x_chain(V, w * m0, k0, k1, seg0_log, 1, true, Vj, Uj);
    const r28::X28 X = reduce_tree8(Vj, Uj);
    const uint32_t j = tid & 7;
    uint8_t* out = j == 0 ? Vout : Uout;
    if (w < (uint32_t)Wg && j < 2 && out) store_jac28(out, tid >> 3, r28::x_to_jac(X));
}

// the same over raw pair-sliced XYZZ records (G2): one chain per lane pair; a lane level after
// level 0 adds U_t too (raw, from the previous lane level).  Outputs raw when the next level is a
// lane level too (raw_out), else Jacobian words (store_jac<PFq2>, the form a row / wave level reads)
template <class F>  // F = Fq2 only
__global__ __launch_bounds__(256) void k_reduce_scaled_r28px(const uint8_t* __restrict__ V, const uint8_t* __restrict__ U,
                                                             uint32_t m_in, uint32_t seg_log, int Wg, int off,
                                                             uint8_t* __restrict__ Vout, uint8_t* __restrict__ Uout,
                                                             int raw_out) {
    MBLS_TAIL_PRIO();
    const uint32_t seg = 1u << seg_log;
    const uint32_t m_out = (m_in + seg - 1) >> seg_log;
    const uint32_t tid = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;  // pair-uniform
    if (tid >= m_out * (uint32_t)Wg) return;
    const uint32_t w = tid / m_out, q = tid % m_out;
    const uint32_t k0 = q << seg_log;
    const uint32_t k1 = min(k0 + seg, m_in);  // exclusive
    const uint32_t base = w * m_in;
    r28p::X28p R = r28p::X28p::inf(), S = r28p::X28p::inf();
    const size_t half = pairdpp::odd() ? 224 : 0;
    uint32_t nw[56];
    load_raw56(V, (size_t)(base + k1 - 1) * 448 + half, nw);
    for (uint32_t t = k1; t-- > k0;) {
        uint32_t cw[56];
#pragma unroll
        for (int i = 0; i < 56; ++i) cw[i] = nw[i];
        if (t > k0) load_raw56(V, (size_t)(base + t - 1) * 448 + half, nw);
        xadd_raw(R, cw);                                                                    // R += V_t
        if ((t - k0) + off != 0 && !R.is_inf()) r28p::xadd(S, R.x, R.y, R.zz, R.zzz);  // S += R
        if (U) {  // S += U_t
            load_raw56(U, (size_t)(base + t) * 448 + half, cw);
            xadd_raw(S, cw);
        }
    }
    if (Vout) {
        // the identity stays exactly zz = 0: a pair product by zz = 0 is only 0 mod p (the partner's
        // negation is a bias multiple of p), which a raw record would carry on as a point
        if (!R.is_inf())
            for (uint32_t k = 0; k < seg_log; ++k) r28p::xdbl(R);
        if (raw_out)
            store_xyzz28p(Vout, tid, R);
        else
            store_jac<PFq2>(Vout, tid, xyzz28p_to_words(R));
    }
    if (raw_out)
        store_xyzz28p(Uout, tid, S);
    else
        store_jac<PFq2>(Uout, tid, xyzz28p_to_words(S));
}

// A narrow level (few segments: the GPU is idle but for one wave per chain) as a tree: one
// workgroup of 4 waves per segment of 4 inputs (off = 0), each wave one wave-layout point op per
// step, intermediate points through LDS.  The same outputs as k_reduce_scaled's chain
//   U' = V1 + 2 V2 + 3 V3 + U0 + U1 + U2 + U3,   V' = 4 (V0 + V1 + V2 + V3)
// in 4 dependent steps instead of 12:
//   1: a = V2 + V3 | b = U0 + U1 | c = U2 + U3 | d = V0 + V1
//   2: e = a + V3  | k = a + V1  | f = b + c   | g = d + a
//   3: W = k + e                               | 2g
//   4: U' = W + f                              | V' = 4g
// (inputs past the level's end are the identity; the additions are exact point additions, so
// the association does not change the resulting point -- only its Jacobian representative,
// which the final (x, y, 1) normalisation removes)
template <class F>
struct TreeLds {
    using J = RJac<F>;
    static constexpr int FQS = RowOf<F>::FQS;  // Fq words-of-12 per coordinate
    static constexpr int WORDS = 3 * FQS * 12;
    MBLS_DEV static void put1(uint32_t* s, const RFq& a) {
        if (wave::row() == 0 && rowdpp::lane16() < 12) s[rowdpp::lane16()] = a.v;
    }
    MBLS_DEV static RFq get1(const uint32_t* s) {
        const uint32_t j = rowdpp::lane16();
        return {j < 12 ? s[j] : 0u};
    }
    MBLS_DEV static void put1(uint32_t* s, const RFq2& a) {
        put1(s, a.c0);
        put1(s + 12, a.c1);
    }
    MBLS_DEV static void get1(const uint32_t* s, RFq2& a) {
        a.c0 = get1(s);
        a.c1 = get1(s + 12);
    }
    MBLS_DEV static void get1(const uint32_t* s, RFq& a) { a = get1(s); }
    MBLS_DEV static void put(uint32_t* s, const J& p) {
        put1(s, p.x);
        put1(s + 12 * FQS, p.y);
        put1(s + 24 * FQS, p.z);
    }
    MBLS_DEV static J get(const uint32_t* s) {
        J p;
        get1(s, p.x);
        get1(s + 12 * FQS, p.y);
        get1(s + 24 * FQS, p.z);
        return p;
    }
};

template <class F>
__global__ __launch_bounds__(256) void k_reduce_tree4(const uint8_t* __restrict__ V, const uint8_t* __restrict__ U,
                                                      uint32_t m_in, uint8_t* __restrict__ Vout,
                                                      uint8_t* __restrict__ Uout) {
    MBLS_TAIL_PRIO();
    using IO = RedIO<F, MODE_WAVE>;
    using J = RJac<F>;
    using T = TreeLds<F>;
    __shared__ uint32_t slot[8][T::WORDS];
    const uint32_t m_out = (m_in + 3) >> 2;
    const uint32_t seg = blockIdx.x;  // grid = m_out * windows exactly
    const uint32_t w = seg / m_out, q = seg % m_out;
    const uint32_t k0 = q << 2, cnt = min(4u, m_in - k0);
    const size_t base = (size_t)w * m_in + k0;
    const int wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto ldV = [&](uint32_t t) { return t < cnt ? IO::ld(V, base + t) : J::inf(); };
    auto ldU = [&](uint32_t t) { return (U && t < cnt) ? IO::ld(U, base + t) : J::inf(); };
    J r = J::inf();
    // steps 1..3 of the additions share one call site (wave-uniform operand selection)
    for (int step = 0; step < 3; ++step) {
        const bool active = step < 2 || wv == 0;
        J x = J::inf(), y = J::inf();
        if (step == 0) {
            x = wv == 0 ? ldV(2) : wv == 1 ? ldU(0) : wv == 2 ? ldU(2) : ldV(0);
            y = wv == 0 ? ldV(3) : wv == 1 ? ldU(1) : wv == 2 ? ldU(3) : ldV(1);
        } else if (step == 1) {
            x = wv == 2 ? T::get(slot[1]) : wv == 3 ? T::get(slot[3]) : T::get(slot[0]);
            y = wv == 0 ? ldV(3) : wv == 1 ? ldV(1) : wv == 2 ? T::get(slot[2]) : T::get(slot[0]);
        } else if (active) {
            x = T::get(slot[5]);  // k
            y = r;                // e
        }
        if (active) r = IO::add(x, y);
        if (step < 2) {
            T::put(slot[4 * step + wv], r);
            __syncthreads();
        }
    }
    if (wv == 0) {
        IO::st(Uout, seg, IO::add(r, T::get(slot[6])));  // U' = W + f
    } else if (wv == 3 && Vout) {
        for (int k = 0; k < 2; ++k) r = IO::dbl(r);  // V' = 4 g
        IO::st(Vout, seg, r);
    }
}

// final fold over window groups: sum_w 2^(c w) G_w  (one chain)
template <class F, int MODE>
MBLS_DEV auto final_fold(const uint8_t* __restrict__ windows, int Wg, int c) {
    using IO = RedIO<F, MODE>;
    auto acc = IO::ld(windows, Wg - 1);
    for (int w = Wg - 2; w >= 0; --w) {
        for (int k = 0; k < c; ++k) acc = IO::dbl(acc);
        acc = IO::add(acc, IO::ld(windows, w));
    }
    return acc;
}
template <class F>
__global__ void k_final(const uint8_t* __restrict__ windows, int Wg, int c, uint8_t* __restrict__ result) {
    MBLS_TAIL_PRIO();
    using IO = RedIO<F, MODE_WAVE>;
    if (IO::id() != 0) return;
    IO::st(result, 0, final_fold<F, MODE_WAVE>(windows, Wg, c));
}

template <class F>
__global__ void k_store_inf(uint8_t* result, int count) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) store_jac<F>(result, i, Jacobian<F>::inf());
}

// ------------------------------------------------------------------------------------
// conversions / utilities
// ------------------------------------------------------------------------------------
MBLS_DEV Fq to_mont_f(const Fq& a) { return to_mont(a); }
MBLS_DEV Fq2 to_mont_f(const Fq2& a) { return {to_mont(a.c0), to_mont(a.c1)}; }
MBLS_DEV Fq from_mont_f(const Fq& a) { return from_mont(a); }
MBLS_DEV Fq2 from_mont_f(const Fq2& a) { return {from_mont(a.c0), from_mont(a.c1)}; }
template <class F>
MBLS_DEV F one_std();
template <>
MBLS_DEV Fq one_std<Fq>() {
    Fq r = Fq::zero();
    r.v[0] = 1;
    return r;
}
template <>
MBLS_DEV Fq2 one_std<Fq2>() {
    Fq2 r = Fq2::zero();
    r.c0.v[0] = 1;
    return r;
}

template <class F>
__global__ void k_points_to_mont(uint8_t* pts, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> p = load_affine<F>(pts, i);
    p.x = to_mont_f(p.x);
    p.y = to_mont_f(p.y);
    store_affine<F>(pts, i, p);
}

// Jacobian Montgomery -> ICICLE standard projective (x, y, 1); identity (0, 1, 0)
// (reference icicle_curve_api.cu:134-229)
MBLS_DEV RFq from_mont_f(const RFq& a) { return from_mont(a); }
MBLS_DEV RFq2 from_mont_f(const RFq2& a) { return {from_mont(a.c0), from_mont(a.c1)}; }
template <>
MBLS_DEV RFq one_std<RFq>() {
    return {rowdpp::lane16() == 0 ? 1u : 0u};
}
template <>
MBLS_DEV RFq2 one_std<RFq2>() {
    return {one_std<RFq>(), RFq::zero()};
}

// one lane per point: the inversion is the binary extended Euclid of mbls_field.hpp (word
// shifts and adds at the full VALU rate; the row-sliced Fermat chain it replaces took 0.29 ms)
// (launched with 64 threads: the bound lets the inversion keep its words in VGPRs -- at the
// default 1024-thread bound it spilled 204 B (G1) / 912 B (G2) to scratch)
template <class F>
MBLS_DEV void icicle_point(const Jacobian<F>& p, uint8_t* out, size_t i) {
    Jacobian<F> o;
    if (p.is_inf()) {
        o.x = F::zero();
        o.y = one_std<F>();
        o.z = F::zero();
    } else {
        Affine<F> a = jac_to_affine(p);
        o.x = from_mont_f(a.x);
        o.y = from_mont_f(a.y);
        o.z = one_std<F>();
    }
    store_jac<F>(out, i, o);
}

// icicle_point on the four lanes of a DPP quad (all active, same p): the inversion runs as
// inv_quad (mbls_binv_quad.hpp); lane 0 of the quad stores
template <class F>
MBLS_DEV void icicle_point_quad(const Jacobian<F>& p, uint8_t* out, size_t i) {
    Jacobian<F> o;
    if (p.is_inf()) {
        o.x = F::zero();
        o.y = one_std<F>();
        o.z = F::zero();
    } else {
        const F zi = inv_quad(p.z);
        const F zi2 = sqr(zi);
        o.x = from_mont_f(p.x * zi2);
        o.y = from_mont_f(p.y * zi2 * zi);
        o.z = one_std<F>();
    }
    if ((__lane_id() & 3u) == 0) store_jac<F>(out, i, o);
}

// in and out may alias (in place)
template <class F>
__global__ __launch_bounds__(64) void k_jac_to_icicle(const uint8_t* in, uint8_t* out, int count) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= count) return;
    icicle_point<F>(load_jac<F>(in, i), out, i);
}

// a row-sliced value (limb j on lane j of every row) gathered into one lane's limbs
MBLS_DEV Fq row_to_lane(const RFq& a) {
    Fq r;
#pragma unroll
    for (int i = 0; i < 12; ++i) r.v[i] = (uint32_t)__shfl((int)a.v, i, 64);
    return r;
}
MBLS_DEV Fq2 row_to_lane(const RFq2& a) { return {row_to_lane(a.c0), row_to_lane(a.c1)}; }

// k_final + k_jac_to_icicle in one launch (single ICICLE MSM, result on device): the wave's
// folded point is gathered into every lane, the first lane quad normalises it (inv_quad) and
// writes ICICLE's (x, y, 1) straight into the caller's buffer (one launch gap and the result
// copy fewer)
template <class F>
__global__ __launch_bounds__(64) void k_final_icicle(const uint8_t* __restrict__ windows, int Wg, int c,
                                                     uint8_t* __restrict__ out) {
    MBLS_TAIL_PRIO();
    const RJac<F> acc = final_fold<F, MODE_WAVE>(windows, Wg, c);
    Jacobian<F> p;
    p.x = row_to_lane(acc.x);
    p.y = row_to_lane(acc.y);
    p.z = row_to_lane(acc.z);
    if (threadIdx.x < 4) icicle_point_quad<F>(p, out, 0);
}

template <class F>
__global__ void k_sum_jac(const uint8_t* pts, int count, uint8_t* out) {
    using IO = RedIO<F, MODE_WAVE>;
    if (IO::id() != 0) return;
    auto acc = RJac<F>::inf();
    for (int i = 0; i < count; ++i) acc = IO::add(acc, IO::ld(pts, i));
    IO::st(out, 0, acc);
}

template <class F>
MBLS_DEV Affine<F> generator();
template <>
MBLS_DEV Affine<Fq> generator<Fq>() { return g1_generator(); }
template <>
MBLS_DEV Affine<Fq2> generator<Fq2>() { return g2_generator(); }

MBLS_DEV uint64_t splitmix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

// scalar i of stream `seed` (same as the oracle's gen_scalar): 4 splitmix64 words, masked to
// 255 bits, minus r once if >= r
MBLS_DEV Fr gen_scalar(uint64_t seed, uint64_t i) {
    uint64_t base = splitmix64(seed) ^ (i * 0xd1342543de82ef95ULL);
    Fr s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint64_t l = splitmix64(base + (uint64_t)j * 0x632be59bd9b4e019ULL);
        if (j == 3) l &= 0x7fffffffffffffffULL;
        s.v[2 * j] = (uint32_t)l;
        s.v[2 * j + 1] = (uint32_t)(l >> 32);
    }
    reduce_once(s);
    return s;
}

// P_i = k_i * G (input generation only; not on the measured path)
template <class F>
__global__ void k_gen_bases(uint8_t* out, uint64_t seed, size_t start, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr k = gen_scalar(seed, start + i);
    Jacobian<F> g = Jacobian<F>::from_affine(generator<F>());
    store_affine<F>(out, i, jac_to_affine(jac_mul_u32(g, k.v)));
}

// precomputed bases, point-major as ICICLE / core/msm.rs:164-165 document:
// out[i*factor + f] = 2^(shift*f) * P_i (Montgomery affine)
template <class F>
__global__ __launch_bounds__(128) void k_precompute(const uint8_t* in, uint8_t* out, size_t n, int factor, int shift) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> a = load_affine<F>(in, i);
    store_affine<F>(out, i * factor, a);
    Jacobian<F> p = Jacobian<F>::from_affine(a);
    for (int f = 1; f < factor; ++f) {
        for (int k = 0; k < shift; ++k) p = jac_dbl(p);
        store_affine<F>(out, i * factor + f, jac_to_affine(p));
    }
}

// ------------------------------------------------------------------------------------
// host orchestration
// ------------------------------------------------------------------------------------
// Tuning knobs in this file are compile-time macros for tools/ variant builds (never run-time
// environment reads: a prover's environment must not select untested kernels).

// the endomorphism images of the bases are built per call (msm_front, into the `phi` block)
inline bool msm_image_table(const MsmPlan& P) { return P.split > 1 && !P.prepared; }
// The one description of an MSM's scratch region: every block in arena order, its bytes and the
// pointer it becomes.  With `base` it carves the region into S; without (the counting pass) S's
// pointers are null.  Either way it returns the region's bytes (a sum of 256-byte multiples).
template <class F>
inline size_t msm_scratch(const MsmPlan& P, uint8_t* base, MsmScratch& S) {
    constexpr size_t jac = PointSize<F>::JAC, aff = PointSize<F>::AFF;
    size_t used = 0;
    auto take = [&](auto*& p, size_t bytes) {
        p = base ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + used) : nullptr;
        used += align_up(bytes);
    };
    const bool psort = partition_sort(P);
    const PartSortSizes ps = psort ? part_sort_sizes(P) : PartSortSizes();  // zero bytes each
    const size_t NC = P.contributions;
    // the chunk count is data dependent (a short last chunk per bucket): its bound
    const uint32_t max_chunks = (uint32_t)(NC / P.chunk + P.TB + 1);
    take(S.keys, 4 * (psort ? 0 : NC));
    take(S.vals, 4 * (psort ? 0 : NC));
    take(S.ranks, 4 * (psort ? 0 : NC));
    take(S.dsrc, digits_src_bytes((uint32_t)(P.split > 1 ? P.pts / P.split : P.pts / P.F), P.split));
    take(S.sorted, 4 * NC);
    const size_t tb_words = (size_t)P.TB + 4;  // + the maximum and the HeavyTab counters
    take(S.counts, 4 * tb_words);
    take(S.offsets, 4 * tb_words);
    take(S.nchunks, 4 * tb_words);
    take(S.chunk_off, 4 * tb_words);
    // + the chunk-count block totals and their prefixes (k_chunk_counts / k_scan_small)
    take(S.tmp,
         4 * (scan_tmp_words(std::max(std::max(max_chunks, P.TB), order_words(P.TB))) + 2 * ((size_t)P.TB / 128 + 2)));
    take(S.owner, 4 * (size_t)max_chunks);
    take(S.first, 4 * (NC / P.chunk + 2));
    take(S.partials, (size_t)max_chunks * xyzz_bytes<F>());
    take(S.buckets, (size_t)P.TB * P.bucket_bytes);
    // V / U ping-pong halves sized for the widest level's outputs (level 0's; msm_device's `half`)
    take(S.levelT, 2 * (size_t)P.level_out[0] * P.Wg * P.level_bytes);
    take(S.levelR, 2 * (size_t)P.level_out[0] * P.Wg * P.level_bytes);
    take(S.windows, (size_t)P.Wg * jac);
    // the per-call image table; with bstride > 1 also the compact copy of the points (2n rows)
    S.phi = nullptr;
    if (msm_image_table(P)) take(S.phi, P.pts / P.split * (P.split - 1 + (P.bstride > 1 ? 1 : 0)) * aff);
    take(S.ent, ps.ent);
    take(S.seg_off, ps.segtab);
    take(S.seg_cnt, ps.segtab);
    take(S.part_tot, ps.parts);
    take(S.ph.help, ps.parts);
    take(S.ph.hh, 4 * (psort ? (size_t)PH_HELPERS * 129 : 0));  // hh[PH_HELPERS][128], then hpart[PH_HELPERS]
    S.ph.hpart = S.ph.hh ? S.ph.hh + (size_t)PH_HELPERS * 128 : nullptr;
    take(S.binhist, 4 * ((size_t)order_words(P.TB) + 1));
    take(S.binbase, 4 * ((size_t)order_words(P.TB) + 1));
    take(S.perm, 4 * (size_t)P.TB);
    // heavy buckets have > SMALL_MAX partials: at most max_chunks / (SMALL_MAX + 1) of them, and
    // at most max_chunks / HEAVY_SLICE + (heavy buckets) slices
    const size_t max_heavy = std::min<size_t>(P.TB, max_chunks / (SMALL_MAX + 1) + 1);
    const size_t max_slices = max_chunks / HEAVY_SLICE + max_heavy + 1;
    take(S.H.bucket, 4 * max_heavy);
    take(S.H.first, 4 * max_heavy);
    take(S.H.nslices, 4 * max_heavy);
    take(S.H.done, 4 * max_heavy);
    take(S.H.owner, 4 * max_slices);
    // slice sums: the planned slices (>= HEAVY_SLICE_MIN partials, <= HEAVY_LDS buckets) or the
    // fixed plan's
    take(S.H.res,
         std::max(max_slices, max_chunks / HEAVY_SLICE_MIN + std::min<size_t>(max_heavy, HEAVY_LDS) + 1) * jac);
    take(S.H.gdone, 4 * (size_t)HEAVY_GDONE);
    S.H.cnt = base ? S.nchunks + P.TB + 1 : nullptr;  // words TB + 1, TB + 2 of the chunk-count array
    return used;
}
template <class F>
inline size_t msm_scratch_bytes(const MsmPlan& P) {
    MsmScratch counted;
    return msm_scratch<F>(P, nullptr, counted);
}

inline bool debug_enabled() {
    static const bool v = [] {
        const char* e = getenv("MBLS_DEBUG");
        return e && atoi(e) != 0;
    }();
    return v;
}

// the accumulation kernel instance
using AccKernel = void (*)(const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t,
                           const uint8_t*, const uint8_t*, uint32_t, uint32_t, uint8_t*);
template <class F>
inline AccKernel accumulate_kernel() {
    if constexpr (std::is_same<F, Fq>::value) return k_accumulate_r28<F>;
    else return k_accumulate_r28p<F>;
}

// contributions per accumulation thread: CHUNK (16), or an eighth of the average bucket when
// buckets are bigger (2^24 points: 1024 contributions per bucket, chunk 128), so a bucket keeps
// <= ~9 partials and its sum stays on the one-thread-per-bucket path (k_bucket_small) -- with
// 16-point chunks every bucket at 2^24 had 64 partials, took the heavy-bucket tree passes and
// the bucket sums cost 93.5 ms against 50.6 ms of accumulation.  Short chunks pay off below
// that: a chunk's first addition is free when the whole wave starts a chunk together (acc = P,
// counter-checked: SQ_INSTS_VALU +5.2% at 86 instead of 16 at 2^20), and spreading NC over one
// round of resident waves (MBLS_ACC_CHUNK=auto, 86 at G1 2^20) cut the bucket sums 0.61 ->
// 0.19 ms but cost 3.25 -> 3.66 ms in the accumulation.
// -DMBLS_ACC_CHUNK=<n> fixes it (variant builds).
#ifndef MBLS_ACC_CHUNK
#define MBLS_ACC_CHUNK 0
#endif
template <class F>
inline uint32_t accumulate_chunk(const MsmPlan& P) {
    if (MBLS_ACC_CHUNK > 0) return (uint32_t)MBLS_ACC_CHUNK;
    const size_t per_bucket = P.contributions / std::max<uint32_t>(P.TB, 1u);
    return (uint32_t)std::max<size_t>(CHUNK, per_bucket / 8);
}

// batch_size > 1: member b's reduction and final fold on a side stream beside member b + 1's
// front and accumulation (TailPipe); 2: member b + 1's front on a second side stream beside member
// b's accumulation as well; 0: every member on the caller's stream (-DMBLS_BATCH_PIPE)
#ifndef MBLS_BATCH_PIPE
#define MBLS_BATCH_PIPE 2
#endif
inline int batch_pipe() { return MBLS_BATCH_PIPE; }

// RED_CHAIN: one level over Wl windows as the generic chain, in the level's mode.  A lane level
// lands here only with Jacobian inputs, which no shipped plan has (plan_levels).
template <class F>
inline void launch_reduce_chain(int mode, const uint8_t* V, const uint8_t* U, uint32_t m_in, uint32_t seg_log, int Wl,
                                int off, uint8_t* Vo, uint8_t* Uo, uint32_t chains, hipStream_t s) {
    switch (mode) {
    case MODE_LANE:
        hipLaunchKernelGGL((k_reduce_scaled<F, MODE_LANE>), dim3((chains * LaneOf<F>::LANES + 255) / 256), dim3(256), 0, s,
                           V, U, m_in, seg_log, Wl, off, Vo, Uo);
        break;
    case MODE_ROW:
        hipLaunchKernelGGL((k_reduce_scaled<F, MODE_ROW>), dim3((chains * 16 + 255) / 256), dim3(256), 0, s, V, U, m_in,
                           seg_log, Wl, off, Vo, Uo);
        break;
    default:
        hipLaunchKernelGGL((k_reduce_scaled<F, MODE_WAVE>), dim3((chains * 64 + 255) / 256), dim3(256), 0, s, V, U, m_in,
                           seg_log, Wl, off, Vo, Uo);
    }
}

// Batch tail pipeline (msm_call, batch_size > 1): member b's reduction levels and final fold --
// latency-bound chains that leave most of the GPU idle -- run on a side stream while member
// b + 1's front and accumulation run on the caller's stream.  The tail reads only the bucket
// sums, the level buffers and the window sums of its member's scratch region (two regions,
// alternating), so the main stream waits for member b - 2's tail (`reuse`) only before it
// writes that region's bucket sums again.
// The front (digits, sort, chunk tables) of member b likewise runs on a second side stream
// beside member b - 1's accumulation: it writes only its own region's front buffers, which member
// b - 2's accumulation and bucket sums read (`front_wait`: that member's bucket_done, or for the
// first two members the fork from the caller's stream).
struct TailPipe {
    hipStream_t side = nullptr;        // the tails run here
    hipEvent_t bucket_done = nullptr;  // recorded on the main stream after the bucket sums
    hipEvent_t reuse = nullptr;        // non-null: the region's previous tail; waited before the bucket sums
    hipStream_t front = nullptr;       // non-null: the front runs here
    hipEvent_t front_wait = nullptr;   // waited on `front` before the member's front
    hipEvent_t front_done = nullptr;   // recorded on `front` after it; the main stream waits on it
};

// Core MSM on device operands: scalars (standard or Montgomery), bases Montgomery affine
// (F*n entries when precomputed); result: one Jacobian Montgomery point on device, or, with
// icicle_out, ICICLE's normalised (x, y, 1) written there by the final fold's launch.
// Everything is enqueued on `st`, one stream-ordered operation that creates no stream and no
// event -- except with `pipe` (the batch pipeline), where the front runs on pipe->front and is
// joined back before the accumulation, and the reduction and the final fold are left on
// pipe->side for the caller to join.
template <class F>
eIcicleError msm_device(const uint8_t* scalars, bool scalars_mont, const uint8_t* bases, uint32_t n,
                        const MsmPlan& P, uint8_t* result, StreamCtx& ctx, hipStream_t st,
                        uint8_t* icicle_out = nullptr, const TailPipe* pipe = nullptr,
                        hipEvent_t acc_event = nullptr) {
    Arena& arena = ctx.arena;
    constexpr size_t AFF = PointSize<F>::AFF;
    constexpr uint32_t LN = LaneOf<F>::LANES;  // lanes per chain in the lane-mode kernels
    // mbls_msm_accumulate_event: recorded after the accumulation launch below, or wherever this
    // function returns before it (an empty MSM, an error)
    AccEventGuard acc_ev(acc_event, st);
    if (n == 0) {
        hipLaunchKernelGGL(k_store_inf<F>, dim3(1), dim3(64), 0, st, result, 1);
        if (icicle_out) hipLaunchKernelGGL(k_jac_to_icicle<F>, dim3(1), dim3(64), 0, st, result, icicle_out, 1);
        MBLS_TRY(hipGetLastError());
        return MBLS_SUCCESS;
    }
    const uint32_t TB = P.TB;
    const size_t NC = P.contributions;
    MsmScratch S;
    uint8_t* region = static_cast<uint8_t*>(arena.take(msm_scratch_bytes<F>(P)));
    if (!region) return MBLS_ALLOCATION_FAILED;
    msm_scratch<F>(P, region, S);

    ProfScope prof_all("msm.total", st);
    eIcicleError er;
    // the front's stream: the caller's, or the batch pipeline's front stream
    const hipStream_t main_st = st;
    if (pipe && pipe->front) {
        if (pipe->front_wait) MBLS_TRY(hipStreamWaitEvent(pipe->front, pipe->front_wait, 0));
        st = pipe->front;
    }
    if ((er = msm_front(scalars, scalars_mont, bases, n, P, S, st)) != MBLS_SUCCESS) return er;
    if (st != main_st) {  // join: the accumulation waits for the front
        MBLS_TRY(hipEventRecord(pipe->front_done, st));
        st = main_st;
        MBLS_TRY(hipStreamWaitEvent(st, pipe->front_done, 0));
    }
    const uint32_t nsplit = msm_image_table(P) ? n : 0xffffffffu;
    {
        // the chunk count is data dependent: launch the bound, extra threads exit
        ProfScope ps("msm.accumulate", st);
        const uint32_t threads = (uint32_t)((NC + P.chunk - 1) / P.chunk) * LN;
        // bstride > 1: the split kernel wrote [P; phi P] into `phi` (compact slot-0 copy)
        const uint8_t* acc_b = P.bstride > 1 ? S.phi : bases;
        const uint8_t* acc_phi = P.bstride > 1 ? S.phi + (size_t)n * AFF : S.phi;
        hipLaunchKernelGGL(accumulate_kernel<F>(), dim3((threads + 255) / 256), dim3(256), 0, st, S.sorted, S.offsets,
                           S.chunk_off, S.first, 0u, TB, acc_b, acc_phi, nsplit, P.chunk, S.partials);
    }
    // mbls_msm_accumulate_event: the tail starts here (the caller passes it to the last member)
    if (hipEvent_t e = acc_ev.release()) MBLS_TRY(hipEventRecord(e, st));
    {
        ProfScope ps("msm.bucket_sum", st);
        // light buckets one thread each, heavy buckets by slice workgroups in the same launch
        // (k_bucket_small); forked heavy passes on a side stream cost ~20 us per event wait,
        // in-line empty passes ~6 us per launch (round 3 timelines)
        const uint32_t light_blocks = (TB * LN + 255) / 256;
        if (pipe && pipe->reuse) MBLS_TRY(hipStreamWaitEvent(st, pipe->reuse, 0));
        hipLaunchKernelGGL(k_bucket_small<F>, dim3(light_blocks + HEAVY_BLOCKS), dim3(256), 0, st, S.chunk_off, S.perm,
                           S.binbase, order_words(TB), S.partials, S.buckets, light_blocks, S.H, P.bucket_raw ? 1 : 0);
    }
    if (pipe) {  // the tail moves to the side stream
        MBLS_TRY(hipEventRecord(pipe->bucket_done, st));
        MBLS_TRY(hipStreamWaitEvent(pipe->side, pipe->bucket_done, 0));
        st = pipe->side;
    }
    {
        ProfScope ps_red("msm.reduce", st);  // the levels only (k_final has its own scope)
        // the plan's launches in order (plan_levels): V / U ping-pong in levelR / levelT by the
        // parity of a launch's last level, whose outputs it writes; the plan's last level writes
        // the window sums straight into `windows`
        const size_t half = (size_t)P.level_out[0] * (size_t)P.Wg * P.level_bytes;
        uint8_t* vb[2] = {S.levelR, S.levelR + half};
        uint8_t* ub[2] = {S.levelT, S.levelT + half};
        const uint8_t* V = S.buckets;
        const uint8_t* U = nullptr;
        for (int k = 0; k < P.launches; ++k) {
            const int l = P.launch[k].level, lo = l + P.launch[k].nlevels - 1;
            const bool last = lo == P.levels - 1;
            uint8_t* Vo = last ? nullptr : vb[lo & 1];
            uint8_t* Uo = last ? S.windows : ub[lo & 1];
            const uint32_t m_in = P.level_m[l], seg_log = P.seg_log[l];
            const uint32_t chains = P.level_out[lo] * (uint32_t)P.Wg;
            const int off = P.off[l];
            switch (P.launch[k].kernel) {
            case RED_TREE4:
                hipLaunchKernelGGL(k_reduce_tree4<F>, dim3(chains), dim3(256), 0, st, V, U, m_in, Vo, Uo);
                break;
            case RED_CHAIN:
                launch_reduce_chain<F>(P.mode[l], V, U, m_in, seg_log, P.Wg, off, Vo, Uo, chains, st);
                break;
            case RED_TREE8:  // the lane keeps its level-0 outputs for the tree: eight lanes per level-1 segment
                if constexpr (!std::is_same<F, Fq>::value) return MBLS_INVALID_ARGUMENT;
                else
                    hipLaunchKernelGGL((k_reduce_tree8_r28x<F>), dim3((8 * chains + 255) / 256), dim3(256), 0, st, V, m_in,
                                       seg_log, P.level_m[lo], P.Wg, Vo, Uo);
                break;
            case RED_R28X:
                if constexpr (!std::is_same<F, Fq>::value) return MBLS_INVALID_ARGUMENT;
                else
                    hipLaunchKernelGGL((k_reduce_scaled_r28x<F>), dim3((chains + 255) / 256), dim3(256), 0, st, V, m_in,
                                       seg_log, P.Wg, off, Vo, Uo);
                break;
            case RED_R28PX:
                if constexpr (!std::is_same<F, Fq2>::value) return MBLS_INVALID_ARGUMENT;
                else
                    hipLaunchKernelGGL((k_reduce_scaled_r28px<F>), dim3((2 * chains + 255) / 256), dim3(256), 0, st, V, U,
                                       m_in, seg_log, P.Wg, off, Vo, Uo, (int)P.raw_out[l]);
                break;
            default:
                return MBLS_INVALID_ARGUMENT;
            }
            V = Vo;
            U = Uo;
        }
    }
    {
        ProfScope ps("msm.final", st);
        if (icicle_out)
            hipLaunchKernelGGL(k_final_icicle<F>, dim3(1), dim3(64), 0, st, S.windows, P.Wg, P.c, icicle_out);
        else
            hipLaunchKernelGGL(k_final<F>, dim3(1), dim3(64), 0, st, S.windows, P.Wg, P.c, result);
    }
    MBLS_TRY(hipGetLastError());
    return MBLS_SUCCESS;
}

// ------------------------------------------------------------------------------------
// boundary wrappers (placement flags, Montgomery flags, batch, ICICLE result format)
// ------------------------------------------------------------------------------------
// entry-point semantics: RAW = the reference's bls12_381_g*_msm_cuda (standard scalars,
// Montgomery bases, flags for placement only, Jacobian Montgomery result, one MSM); ICICLE =
// msm_cuda_impl (Montgomery flags honoured, batch, (x, y, 1) standard result); JACOBIAN = ICICLE
// inputs with the Jacobian Montgomery result left unnormalised (the per-rank step of the
// sharded multi-GPU MSM: partials are summed before the one normalisation)
enum MsmEntry : int { MSM_RAW = 0, MSM_ICICLE = 1, MSM_JACOBIAN = 2 };

template <class F>
eIcicleError msm_call(const void* scalars, const void* bases, int msm_size, const MSMConfig* cfg, void* results,
                      int entry) {
    const bool icicle_semantics = entry != MSM_RAW;
    constexpr size_t AFF = PointSize<F>::AFF, JAC = PointSize<F>::JAC;
    if (!cfg || !results) return MBLS_INVALID_POINTER;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    // a pending mbls_msm_accumulate_event belongs to this call whatever happens below: the last
    // member's accumulation records it (msm_device), any earlier return records it here
    AccEventGuard acc_ev(take_accumulate_event(st), st);
    if (msm_size < 0 || msm_size > (1 << MAX_MSM_LOG)) return MBLS_INVALID_ARGUMENT;
    if (msm_size > 0 && (!scalars || !bases)) return MBLS_INVALID_POINTER;
    const int batch = icicle_semantics ? (cfg->batch_size > 0 ? cfg->batch_size : 1) : 1;
    // The reference's plain device-bases MSMs (core/msm.rs:897-913, 1025-1040, 1097-1110) set
    // cfg.precompute_factor = MIDNIGHT_GPU_PRECOMPUTE on a buffer of n plain bases; its backend
    // never reads the factor.  A device allocation too short for n x F table entries cannot be a
    // precompute_bases table: it runs as factor 1, the reference's result (the
    // binding should pass PrecomputedBases::factor()).
    // Strict mode (mbls_msm_precompute_strict(1), for a binding that cannot pass the table's own
    // factor): only a table precompute_bases wrote (registered, same factor, covering the call)
    // runs as a table; anything else is plain bases -- exact for sub-allocated buffers too.
    MSMConfig cfg_plain;
    if (cfg->precompute_factor > 1 && cfg->are_points_on_device && bases && msm_size > 0) {
        const bool sh = cfg->are_points_shared_in_batch || batch == 1;
        const size_t want = (size_t)msm_size * (size_t)cfg->precompute_factor * (sh ? 1 : (size_t)batch) *
                            AFF;
        if (precompute_strict() ? !precompute_is_table(bases, cfg->precompute_factor, want)
                                : device_bytes_from(bases) < want) {
            cfg_plain = *cfg;
            cfg_plain.precompute_factor = 1;
            cfg = &cfg_plain;
        }
    }
    MsmPlan P;
    eIcicleError er = make_plan(msm_size > 0 ? msm_size : 1, cfg, P, std::is_same<F, Fq>::value ? 2 : 4);
    if (er != MBLS_SUCCESS) return er;
    const bool scal_mont = icicle_semantics ? cfg->are_scalars_montgomery_form : false;
    // a precomputed table (F > 1) is precompute_call output, Montgomery whatever the flag says:
    // core/msm.rs:641-643 passes are_bases_montgomery_form = !is_precomputed() = false with it
    const bool pts_mont = icicle_semantics && P.table == 1 ? cfg->are_points_montgomery_form : true;
    const bool shared = cfg->are_points_shared_in_batch || batch == 1;
    const size_t n = (size_t)msm_size;
    const size_t nbases_per = n * (size_t)P.table;
    const size_t nbases = shared ? nbases_per : nbases_per * batch;

    CtxLease lease(st);
    if (!lease) return lease.error();
    StreamCtx& ctx = *lease;
    Arena& A = ctx.arena;
    size_t st_s = (!cfg->are_scalars_on_device) ? align_up(n * 32 * batch) : 0;
    size_t st_b = (!cfg->are_points_on_device || !pts_mont) ? align_up(nbases * AFF) : 0;
    size_t st_r = align_up(JAC * (size_t)batch);
    P.chunk = accumulate_chunk<F>(P);
    if (debug_enabled())
        fprintf(stderr, "[mbls] msm n=%d c=%d W=%d Wg=%d split=%d TB=%u contributions=%zu chunk=%u levels=%d\n", msm_size,
                P.c, P.W, P.Wg, P.split, P.TB, P.contributions, P.chunk, P.levels);
    const size_t scratch = msm_scratch_bytes<F>(P);
    const bool piped = batch > 1 && batch_pipe() > 0;
    er = lease.reserve(st_s + st_b + st_r + scratch * (piped ? 2 : 1) + 4096);
    if (er != MBLS_SUCCESS) return er;

    const uint8_t* d_s = static_cast<const uint8_t*>(scalars);
    const uint8_t* d_b = static_cast<const uint8_t*>(bases);
    if (st_s) {
        // host scalars (core/msm.rs:665,773 pass a HostSlice): stream-ordered; a pageable buffer is
        // out of the caller's memory when hipMemcpyAsync returns, a pinned one is the caller's to
        // keep alive until the stream completes (as in ICICLE).
        // Pinned memory whose first kernel reads each scalar exactly once (the GLV / psi split, or
        // the Montgomery -> standard conversion) is read in place over PCIe through its device
        // alias: the front kernel overlaps the transfer with its own work and no 32 MiB staging
        // copy is written and re-read.  Otherwise: a PCIe copy kernel (pinned)
        // or hipMemcpyAsync (pageable, or another device's memory for multi-device shards).
        const bool read_once = P.split > 1 || scal_mont;
        const void* alias = read_once ? pinned_host_device_pointer(scalars) : nullptr;
        if (alias) {
            d_s = static_cast<const uint8_t*>(alias);
        } else {
            void* t = A.take(n * 32 * batch);
            if ((er = stage_to_device(t, scalars, n * 32 * batch, st)) != MBLS_SUCCESS) return er;
            d_s = static_cast<const uint8_t*>(t);
        }
    }
    if (st_b) {
        void* t = A.take(nbases * AFF);
        if (cfg->are_points_on_device) {
            MBLS_TRY(hipMemcpyAsync(t, bases, nbases * AFF, hipMemcpyDefault, st));
        } else if ((er = stage_to_device(t, bases, nbases * AFF, st)) != MBLS_SUCCESS) {
            return er;
        }
        if (!pts_mont) {
            hipLaunchKernelGGL(k_points_to_mont<F>, dim3((unsigned)((nbases + 255) / 256)), dim3(256), 0, st,
                               (uint8_t*)t, nbases);
            MBLS_TRY(hipGetLastError());
        }
        d_b = static_cast<const uint8_t*>(t);
    }
    uint8_t* d_r = static_cast<uint8_t*>(A.take(JAC * (size_t)batch));
    // one ICICLE MSM with its result on the device: the final fold writes the normalised
    // (x, y, 1) straight into `results` (k_final_icicle; 16-byte stores, so aligned buffers only)
    uint8_t* direct = (entry == MSM_ICICLE && batch == 1 && cfg->are_results_on_device &&
                       ((uintptr_t)results & 15) == 0)
                          ? (uint8_t*)results
                          : nullptr;
    const size_t mark = A.mark();
    // side streams: 0 the tails, 1 the fronts; events: 0-1 bucket_done, 2-3 tail done, 4-5 front
    // done, 6 the fork (per region where paired)
    if (piped && (er = ctx.ensure_side(7, 2)) != MBLS_SUCCESS) return er;
    if (piped) {
        ctx.forked = true;
        MBLS_TRY(hipEventRecord(ctx.events[6], st));
    }
    for (int b = 0; b < batch; ++b) {
        // scratch reused across the batch (stream-ordered); piped: two regions, alternating
        A.rewind(mark);
        TailPipe pipe;
        if (piped) {
            if ((b & 1) && !A.take(scratch)) return MBLS_ALLOCATION_FAILED;
            pipe.side = ctx.sides[0];
            pipe.bucket_done = ctx.events[b & 1];
            pipe.reuse = b >= 2 ? ctx.events[2 + (b & 1)] : nullptr;
            pipe.front = batch_pipe() > 1 ? ctx.sides[1] : nullptr;
            pipe.front_wait = b >= 2 ? ctx.events[b & 1] : ctx.events[6];
            pipe.front_done = ctx.events[4 + (b & 1)];
        }
        const uint8_t* sb = d_s + (size_t)b * n * 32;
        const uint8_t* bb = d_b + (shared ? 0 : (size_t)b * nbases_per * AFF);
        // piped ICICLE members are normalised inside their tails (hidden but for the last one)
        uint8_t* icicle_b = direct ? direct : (piped && entry == MSM_ICICLE ? d_r + (size_t)b * JAC : nullptr);
        er = msm_device<F>(sb, scal_mont, bb, (uint32_t)n, P, d_r + (size_t)b * JAC, ctx, st, icicle_b,
                           piped ? &pipe : nullptr, b == batch - 1 ? acc_ev.release() : nullptr);
        if (er != MBLS_SUCCESS) return er;
        if (piped) MBLS_TRY(hipEventRecord(ctx.events[2 + (b & 1)], pipe.side));
    }
    // the side stream runs the tails in member order: its last event covers them all
    if (piped) MBLS_TRY(hipStreamWaitEvent(st, ctx.events[2 + ((batch - 1) & 1)], 0));
    // every side stream is joined into `st` by now (the fronts' front_done, the tails' last
    // event above): only an early error return leaves
    // the lease's fallback join to do
    ctx.forked = false;
    if (!direct) {
        if (entry == MSM_ICICLE && !piped) {
            hipLaunchKernelGGL(k_jac_to_icicle<F>, dim3((batch + 63) / 64), dim3(64), 0, st, d_r, d_r, batch);
            MBLS_TRY(hipGetLastError());
        }
        MBLS_TRY(hipMemcpyAsync(results, d_r, JAC * (size_t)batch,
                                cfg->are_results_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    }
    MBLS_TRY(hipGetLastError());
    // is_async is honoured whatever the input placement (staged inputs live in the leased
    // context, which later calls only reuse after this call's `done` event); a host result needs
    // the wait
    if (!cfg->is_async || !cfg->are_results_on_device) MBLS_TRY(hipStreamSynchronize(st));
    return MBLS_SUCCESS;
}

// ------------------------------------------------------------------------------------
// multi-device MSM for a single-process caller (mbls_g*_msm_multi_device): SURVEY.md 8e's
// shard -> partial -> exchange -> EC sum -> one normalisation, with the exchange as peer copies
// of the 144 / 288-byte Jacobian partials to the first device (RCCL's reduce ops cannot add
// curve points; the torch.distributed path of bench.py / sharded_msm.py all-gathers them).
// ------------------------------------------------------------------------------------
static constexpr int MAX_SHARDS = 64;
struct MultiDevRes {  // per device, created once, used under the multi-device lock
    hipStream_t stream = nullptr;
    hipEvent_t ev[MAX_SHARDS] = {};
    uint8_t* partials = nullptr;  // MAX_SHARDS Jacobian partials (G2 size)
    uint8_t* gather = nullptr;    // (first device) MAX_SHARDS gathered partials + the sum
    hipEvent_t done = nullptr;    // (first device) recorded on the call's first stream at its end
};
std::mutex& multi_device_mutex();
// the first device's resources of the last call (its `done` orders the next call's reuse of the
// partial / gather slots, whatever streams the two calls use); under the multi-device lock
MultiDevRes*& multi_device_last();
eIcicleError multi_device_res(int dev, MultiDevRes*& out);
eIcicleError enable_peer(int from, int to);

template <class F>
eIcicleError msm_multi_device(const void* scalars, const void* const* bases_per_dev, const int* devs, int ndev,
                              int msm_size, const MSMConfig* cfg, void* result) {
    constexpr size_t JAC = PointSize<F>::JAC;
    if (!cfg || !result || !devs || !bases_per_dev) return MBLS_INVALID_POINTER;
    if (ndev < 1 || ndev > MAX_SHARDS || msm_size < 0 || msm_size > (1 << MAX_MSM_LOG)) return MBLS_INVALID_ARGUMENT;
    if (cfg->batch_size > 1 || cfg->precompute_factor > 1) return MBLS_INVALID_ARGUMENT;
    if (msm_size > 0 && !scalars) return MBLS_INVALID_POINTER;
    int count = 0;
    MBLS_TRY(hipGetDeviceCount(&count));
    for (int k = 0; k < ndev; ++k) {
        if (devs[k] < 0 || devs[k] >= count) return MBLS_INVALID_DEVICE;
        if (msm_size > 0 && !bases_per_dev[k]) return MBLS_INVALID_POINTER;
    }
    int cur = 0;
    MBLS_TRY(hipGetDevice(&cur));
    std::lock_guard<std::mutex> lk(multi_device_mutex());
    struct Restore {
        int d;
        ~Restore() { (void)hipSetDevice(d); }
    } restore{cur};
    const int d0 = devs[0];
    MultiDevRes* r0 = nullptr;
    eIcicleError er = multi_device_res(d0, r0);
    if (er != MBLS_SUCCESS) return er;
    for (int k = 1; k < ndev; ++k) {  // both directions: scalars d0 -> d, the partial d -> d0
        if ((er = enable_peer(d0, devs[k])) != MBLS_SUCCESS) return er;
        if ((er = enable_peer(devs[k], d0)) != MBLS_SUCCESS) return er;
    }
    hipStream_t st0 = cfg->stream ? static_cast<hipStream_t>(cfg->stream) : r0->stream;
    // shard streams are forked from the caller's stream: the caller's earlier work on its
    // inputs (a device scalar upload, say) is ordered before every shard
    MBLS_TRY(hipSetDevice(d0));
    // a pending mbls_msm_accumulate_event of the caller's stream: taken here (so the first shard's
    // msm_call on st0 does not), recorded on st0 when this call returns
    AccEventGuard acc_ev(take_accumulate_event(st0), st0);
    // the previous call may still read or write the partial / gather slots on its own streams
    // (is_async with a caller stream): this call's fork -- and so every shard -- waits for its end
    if (MultiDevRes* last = multi_device_last()) MBLS_TRY(hipStreamWaitEvent(st0, last->done, 0));
    MBLS_TRY(hipEventRecord(r0->ev[MAX_SHARDS - 1], st0));
    const size_t n = (size_t)msm_size;
    for (int k = 0; k < ndev; ++k) {
        const int d = devs[k];
        MultiDevRes* r = nullptr;
        if ((er = multi_device_res(d, r)) != MBLS_SUCCESS) return er;
        MBLS_TRY(hipSetDevice(d));
        hipStream_t sk = (d == d0) ? st0 : r->stream;
        if (sk != st0) MBLS_TRY(hipStreamWaitEvent(sk, r0->ev[MAX_SHARDS - 1], 0));
        const size_t lo = n * (size_t)k / ndev, hi = n * (size_t)(k + 1) / ndev;
        MSMConfig c = *cfg;
        c.stream = sk;
        c.batch_size = 1;
        c.are_results_on_device = true;
        c.is_async = true;
        // scalars on another device than the shard's: staged (a peer copy, hipMemcpyDefault)
        c.are_scalars_on_device = cfg->are_scalars_on_device && d == d0;
        const uint8_t* sp = static_cast<const uint8_t*>(scalars) + lo * 32;
        er = msm_call<F>(hi > lo ? sp : nullptr, bases_per_dev[k], (int)(hi - lo), &c, r->partials + (size_t)k * JAC,
                         MSM_JACOBIAN);
        if (er != MBLS_SUCCESS) return er;
        MBLS_TRY(hipEventRecord(r->ev[k], sk));
    }
    // exchange: the partials to the first device, then one EC sum and one normalisation
    MBLS_TRY(hipSetDevice(d0));
    for (int k = 0; k < ndev; ++k) {
        MultiDevRes* r = nullptr;
        if ((er = multi_device_res(devs[k], r)) != MBLS_SUCCESS) return er;
        if (devs[k] != d0) MBLS_TRY(hipStreamWaitEvent(st0, r->ev[k], 0));
        MBLS_TRY(hipMemcpyPeerAsync(r0->gather + (size_t)k * JAC, d0, r->partials + (size_t)k * JAC, devs[k], JAC, st0));
    }
    uint8_t* sum = r0->gather + (size_t)MAX_SHARDS * JAC;
    hipLaunchKernelGGL(k_sum_jac<F>, dim3(1), dim3(64), 0, st0, r0->gather, ndev, sum);
    hipLaunchKernelGGL(k_jac_to_icicle<F>, dim3(1), dim3(64), 0, st0, sum, sum, 1);
    MBLS_TRY(hipGetLastError());
    MBLS_TRY(hipMemcpyAsync(result, sum, JAC, cfg->are_results_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                            st0));
    // the library's per-device resources are reused by the next call: it waits for `done`
    MBLS_TRY(hipEventRecord(r0->done, st0));
    multi_device_last() = r0;
    if (!cfg->is_async || !cfg->are_results_on_device || !cfg->stream) MBLS_TRY(hipStreamSynchronize(st0));
    return MBLS_SUCCESS;
}

// ICICLE precompute_bases (registered MsmPreComputeImpl, icicle_backend_api.cuh:188-193; the
// reference's icicle_curve_api.cu:415-440 is a plain byte copy, so its factor > 1 is wrong).
// out[i*F + f] = 2^(s f) P_i, s = precompute_shift(F) = ceil(256 / F): the shift depends on the
// factor only, so one table serves an MSM of any c (MIDNIGHT_MSM_WINDOW or auto) and any
// msm_size <= bases_size, as core/msm.rs:441-454 -> :630-650 uses it.  The output is always
// Montgomery affine; standard-form input (are_points_montgomery_form = false) is converted.
template <class F>
eIcicleError precompute_call(const void* in, int n, const MSMConfig* cfg, void* out) {
    constexpr size_t AFF = PointSize<F>::AFF;
    if (!cfg || !in || !out) return MBLS_INVALID_POINTER;
    if (n < 0) return MBLS_INVALID_ARGUMENT;
    const int factor = cfg->precompute_factor > 0 ? cfg->precompute_factor : 1;
    if (factor > MAX_PRECOMPUTE) return MBLS_INVALID_ARGUMENT;
    if (n == 0) return MBLS_SUCCESS;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    CtxLease lease(st);
    if (!lease) return lease.error();
    Arena& A = lease->arena;
    size_t in_b = (size_t)n * AFF, out_b = in_b * factor;
    eIcicleError er = lease.reserve(align_up(in_b) + align_up(out_b));
    if (er != MBLS_SUCCESS) return er;
    uint8_t* din = (uint8_t*)A.take(in_b);
    uint8_t* dout = (uint8_t*)A.take(out_b);
    MBLS_TRY(hipMemcpyAsync(din, in, in_b, cfg->are_points_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (!cfg->are_points_montgomery_form)
        hipLaunchKernelGGL(k_points_to_mont<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, din, (size_t)n);
    // the factor equal to the group's endomorphism split prepares the image table instead
    // (make_plan: an MSM with that factor splits its scalars against it)
    constexpr int endo = std::is_same<F, Fq>::value ? 2 : 4;
    if (factor == endo) {
        if ((er = launch_endo_table(din, dout, (uint32_t)n, endo, st)) != MBLS_SUCCESS) return er;
    } else {
        hipLaunchKernelGGL(k_precompute<F>, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, din, dout, (size_t)n,
                           factor, precompute_shift(factor));
    }
    MBLS_TRY(hipGetLastError());
    MBLS_TRY(hipMemcpyAsync(out, dout, out_b, cfg->are_results_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    MBLS_TRY(hipStreamSynchronize(st));
    if (cfg->are_results_on_device) precompute_register(out, out_b, factor);  // strict mode's table list
    return MBLS_SUCCESS;
}

}  // namespace mbls
