// mbls_scan.hpp -- the Fr scan skeleton shared by scan.hip (grand product, Horner) and logup.hip
// (running sum): geometry, operators, the tile scan and the three launches.
//
// One skeleton, three operators, three plain launches on the caller's stream:
//   1. k_scan_reduce      each workgroup folds its span (a whole number of tiles) to one aggregate;
//   2. k_scan_aggregates  one workgroup per batch member scans the <= 1024 span aggregates into the
//                         value entering each span, and writes the member's total;
//   3. k_scan_write       each workgroup re-reads its span and writes the scanned elements, starting
//                         from the value entering the span.
// No workgroup ever waits for another one: no look-back, no flags in global memory, no cooperative
// launch.  The price is the second read of the input: 96 B per element instead of 64 B.
//
// The operators advance a running value over a piece with at most ONE Montgomery product:
//   mul     run -> run * x
//   horner  run -> x + m * run, m = z^(length of the piece), x = the piece's own Horner value
//   add     run -> run + x      (one modular addition, no product and no multiplier)
// (the scan runs right to left for horner).  A piece's multiplier depends on its length only, so a
// Kogge-Stone step at distance d uses one uniform multiplier z^(K d), obtained by squaring: no pair
// of field elements is carried.  Elements past the end of a member read as the operator's identity
// (one / zero), which leaves every real output as it is, so a partial chunk, tile or span needs no
// case of its own.
//
// Scan inputs are witness-derived: no branch and no address below depends on a field value; the
// conditions are on thread, lane, tile and size only.
#pragma once
#include <hip/hip_runtime.h>

#include "mbls_common.hpp"
#include "mbls_field.hpp"

namespace mbls {

// ---- geometry: the tile constants live here and nowhere else (mbls_fr_scan_geometry reports them)
#ifndef MBLS_SCAN_K
#define MBLS_SCAN_K 8
#endif
static constexpr int SCAN_K = MBLS_SCAN_K;  // contiguous elements per thread, held in registers
static constexpr int SCAN_THREADS = 256;
static constexpr int SCAN_WAVE = 64;
static constexpr int SCAN_WAVES = SCAN_THREADS / SCAN_WAVE;
static constexpr int SCAN_TILE = SCAN_K * SCAN_THREADS;  // elements a workgroup scans per step
static constexpr int SCAN_AGG_K = 4;                     // span aggregates per thread in launch 2
static constexpr int SCAN_MAX_GROUPS = SCAN_AGG_K * SCAN_THREADS;
static constexpr size_t SCAN_MAX_ELEMS = (size_t)1 << 26;
static_assert((SCAN_K & (SCAN_K - 1)) == 0 && (SCAN_AGG_K & (SCAN_AGG_K - 1)) == 0, "z^K by squaring");

struct ScanGeom {
    size_t span;      // elements per workgroup: tiles_per_group * SCAN_TILE
    uint32_t groups;  // workgroups per member, <= SCAN_MAX_GROUPS
    uint32_t tiles_per_group;
};
static ScanGeom scan_geom(size_t size) {
    const size_t tiles = (size + SCAN_TILE - 1) / SCAN_TILE;
    ScanGeom g;
    g.tiles_per_group = (uint32_t)((tiles + SCAN_MAX_GROUPS - 1) / SCAN_MAX_GROUPS);
    if (g.tiles_per_group == 0) g.tiles_per_group = 1;
    g.span = (size_t)g.tiles_per_group * SCAN_TILE;
    g.groups = (uint32_t)((size + g.span - 1) / g.span);
    if (g.groups == 0) g.groups = 1;
    return g;
}

// ---- the operators.  step(run, x, m): the value after the piece x, entered with `run`; m is the
// multiplier of the piece x (read by horner only)
struct ScanMul {
    static constexpr bool REV = false;   // scans left to right
    static constexpr bool POWERS = false;
    MBLS_DEV static Fr identity() { return Fr::one(); }
    MBLS_DEV static Fr step(const Fr& run, const Fr& x, const Fr&) { return run * x; }
};
struct ScanHorner {
    static constexpr bool REV = true;    // scans right to left
    static constexpr bool POWERS = true;
    MBLS_DEV static Fr identity() { return Fr::zero(); }
    MBLS_DEV static Fr step(const Fr& run, const Fr& x, const Fr& m) { return x + m * run; }
};
struct ScanAdd {
    static constexpr bool REV = false;
    static constexpr bool POWERS = false;
    MBLS_DEV static Fr identity() { return Fr::zero(); }
    MBLS_DEV static Fr step(const Fr& run, const Fr& x, const Fr&) { return run + x; }
};

MBLS_DEV uint32_t lane_mask(bool c) { return 0u - (uint32_t)c; }

// the value of the lane `d` places earlier in scan order (its own value where there is none)
template <bool REV>
MBLS_DEV Fr shfl_prev(const Fr& v, int d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = REV ? __shfl_down(v.v[i], d, SCAN_WAVE) : __shfl_up(v.v[i], d, SCAN_WAVE);
    return r;
}

template <int LOG>
MBLS_DEV Fr pow_2k(Fr a) {
#pragma unroll
    for (int i = 0; i < LOG; ++i) a = sqr(a);
    return a;
}
constexpr int ilog2(int x) { return x <= 1 ? 0 : 1 + ilog2(x / 2); }

// a^e for an exponent that depends on the launch geometry or the lane, never on data
MBLS_DEV Fr pow_public(const Fr& a, uint64_t e, int bits) {
    Fr acc = Fr::one();
    for (int b = bits - 1; b >= 0; --b) {
        acc = sqr(acc);
        acc = fr_select(lane_mask((e >> b) & 1), acc * a, acc);
    }
    return acc;
}

// the per-thread constants of a launch: the element multiplier (horner: z for launches 1 and 3,
// z^span for launch 2), its KK-th power (a thread's chunk) and the power for the `rank` chunks
// before this lane in its wave
struct ScanPowers {
    Fr unit, chunk, lane;
};
template <class Op, int KK>
MBLS_DEV ScanPowers scan_powers(const Fr& unit) {
    ScanPowers p;
    p.unit = unit;
    if constexpr (Op::POWERS) {
        const int lane = threadIdx.x & (SCAN_WAVE - 1);
        p.chunk = pow_2k<ilog2(KK)>(unit);
        p.lane = pow_public(p.chunk, (uint64_t)(Op::REV ? SCAN_WAVE - 1 - lane : lane), ilog2(SCAN_WAVE));
    } else {
        p.chunk = p.lane = unit;
    }
    return p;
}

// One tile: thread t holds x[0 .. KK) = elements t*KK .. t*KK + KK - 1 of the tile.  `run` is the
// value entering the tile and becomes the value leaving it.  Returns the value entering this
// thread's chunk (CARRY), or nothing of use.  `sh`: SCAN_WAVES elements of LDS, free until the
// caller's next barrier but one (callers alternate between two such buffers).
template <class Op, int KK, bool CARRY>
MBLS_DEV Fr tile_scan(const Fr (&x)[KK], const ScanPowers& pw, Fr& run, uint8_t* sh) {
    constexpr bool REV = Op::REV;
    const int lane = threadIdx.x & (SCAN_WAVE - 1), wave = threadIdx.x / SCAN_WAVE;
    const int rank = REV ? SCAN_WAVE - 1 - lane : lane;            // this lane's place in scan order
    const int wrank = REV ? SCAN_WAVES - 1 - wave : wave;
    // the thread folds its chunk serially
    Fr v = x[REV ? KK - 1 : 0];
#pragma unroll
    for (int k = 1; k < KK; ++k) v = Op::step(v, x[REV ? KK - 1 - k : k], pw.unit);
    // Kogge-Stone across the wave: after the step at distance d, v covers the (up to) 2d chunks
    // ending at this lane; the fetched value is d whole chunks or nothing, so m = chunk^d serves all
    Fr m = pw.chunk;
#pragma unroll
    for (int d = 1; d < SCAN_WAVE; d <<= 1) {
        const Fr u = fr_select(lane_mask(rank >= d), shfl_prev<REV>(v, d), Op::identity());
        v = Op::step(u, v, m);
        if constexpr (Op::POWERS) m = sqr(m);
    }
    // m = chunk^64, the multiplier of a whole wave
    Fr before = Op::identity();
    if constexpr (CARRY) before = fr_select(lane_mask(rank >= 1), shfl_prev<REV>(v, 1), Op::identity());
    if (rank == SCAN_WAVE - 1) store<FrCfg>(sh + 32 * wave, v);
    __syncthreads();
    // the waves' aggregates, in scan order, on top of the value entering the tile
    Fr acc = run, wave_in = run;
#pragma unroll
    for (int j = 0; j < SCAN_WAVES; ++j) {
        if (j == wrank) wave_in = acc;
        acc = Op::step(acc, load<FrCfg>(sh + 32 * (REV ? SCAN_WAVES - 1 - j : j)), m);
    }
    run = acc;
    if constexpr (CARRY) return Op::step(wave_in, before, pw.lane);  // `before` spans `rank` chunks
    return wave_in;
}

// a thread's chunk of the member `in` (size elements) from element `base` on; identity past the end
template <class Op, int KK>
MBLS_DEV void load_chunk(Fr (&x)[KK], const uint8_t* in, size_t base, size_t size) {
    if (base + KK <= size) {
#pragma unroll
        for (int k = 0; k < KK; ++k) x[k] = load<FrCfg>(in + 32 * (base + k));
    } else {
#pragma unroll
        for (int k = 0; k < KK; ++k) {
            x[k] = Op::identity();
            if (base + k < size) x[k] = load<FrCfg>(in + 32 * (base + k));
        }
    }
}

// tiles of span `grp` that hold elements of the member
MBLS_DEV uint32_t span_tiles(const ScanGeom& g, uint32_t grp, size_t size) {
    const size_t left = size - (size_t)grp * g.span;  // > 0: groups = ceil(size / span)
    const size_t t = (left + SCAN_TILE - 1) / SCAN_TILE;
    return t < g.tiles_per_group ? (uint32_t)t : g.tiles_per_group;
}

// ---- launch 1: agg[member * groups + grp] = the span's aggregate (entered with the identity)
template <class Op>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_reduce(uint8_t* __restrict__ agg, const uint8_t* __restrict__ in,
                                                              const uint8_t* __restrict__ zs, size_t size, ScanGeom g) {
    __shared__ __attribute__((aligned(16))) uint8_t sh[2 * SCAN_WAVES * 32];
    const uint32_t member = blockIdx.x / g.groups, grp = blockIdx.x % g.groups;
    in += 32 * size * (size_t)member;
    const ScanPowers pw = scan_powers<Op, SCAN_K>(Op::POWERS ? load<FrCfg>(zs + 32 * (size_t)member) : Fr::one());
    const uint32_t nt = span_tiles(g, grp, size);
    Fr run = Op::identity();
    for (uint32_t i = 0; i < nt; ++i) {
        const uint32_t t = Op::REV ? nt - 1 - i : i;
        Fr x[SCAN_K];
        load_chunk<Op, SCAN_K>(x, in, (size_t)grp * g.span + (size_t)t * SCAN_TILE + (size_t)threadIdx.x * SCAN_K, size);
        tile_scan<Op, SCAN_K, false>(x, pw, run, sh + (i & 1) * SCAN_WAVES * 32);
    }
    if (threadIdx.x == 0) store<FrCfg>(agg + 32 * (size_t)blockIdx.x, run);
}

// ---- launch 2, one workgroup per member: carry[member * groups + grp] = the value entering span
// grp, total[member] = the value leaving the member (either output may be null)
template <class Op>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_aggregates(uint8_t* __restrict__ carry, uint8_t* __restrict__ total,
                                                                  const uint8_t* __restrict__ agg,
                                                                  const uint8_t* __restrict__ zs,
                                                                  const uint8_t* __restrict__ init, ScanGeom g) {
    __shared__ __attribute__((aligned(16))) uint8_t sh[SCAN_WAVES * 32];
    const size_t member = blockIdx.x;
    agg += 32 * member * g.groups;
    // one element of this scan is a whole span: its multiplier is z^span
    Fr unit = Fr::one();
    if constexpr (Op::POWERS) unit = pow_public(load<FrCfg>(zs + 32 * member), g.span, 32);
    const ScanPowers pw = scan_powers<Op, SCAN_AGG_K>(unit);
    Fr x[SCAN_AGG_K];
    const size_t base = (size_t)threadIdx.x * SCAN_AGG_K;
    load_chunk<Op, SCAN_AGG_K>(x, agg, base, g.groups);
    Fr run = Op::identity();
    if (init) run = load<FrCfg>(init + 32 * member);
    Fr cur = tile_scan<Op, SCAN_AGG_K, true>(x, pw, run, sh);
    if (carry) {
#pragma unroll
        for (int k = 0; k < SCAN_AGG_K; ++k) {
            const int kk = Op::REV ? SCAN_AGG_K - 1 - k : k;
            if (base + kk < g.groups) store<FrCfg>(carry + 32 * (member * g.groups + base + kk), cur);
            cur = Op::step(cur, x[kk], pw.unit);
        }
    }
    if (total && threadIdx.x == 0) store<FrCfg>(total + 32 * member, run);
}

// ---- launch 3: out[i] = the value entering element i (INCLUSIVE: leaving it).  Every element is
// read into registers by the thread that later writes it, so out may be in.
template <class Op, bool INCLUSIVE>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_write(uint8_t* __restrict__ out, const uint8_t* in,
                                                             const uint8_t* __restrict__ carry,
                                                             const uint8_t* __restrict__ zs, size_t size, ScanGeom g) {
    __shared__ __attribute__((aligned(16))) uint8_t sh[2 * SCAN_WAVES * 32];
    const uint32_t member = blockIdx.x / g.groups, grp = blockIdx.x % g.groups;
    in += 32 * size * (size_t)member;
    out += 32 * size * (size_t)member;
    const ScanPowers pw = scan_powers<Op, SCAN_K>(Op::POWERS ? load<FrCfg>(zs + 32 * (size_t)member) : Fr::one());
    const uint32_t nt = span_tiles(g, grp, size);
    Fr run = load<FrCfg>(carry + 32 * (size_t)blockIdx.x);
    for (uint32_t i = 0; i < nt; ++i) {
        const uint32_t t = Op::REV ? nt - 1 - i : i;
        const size_t base = (size_t)grp * g.span + (size_t)t * SCAN_TILE + (size_t)threadIdx.x * SCAN_K;
        Fr x[SCAN_K];
        load_chunk<Op, SCAN_K>(x, in, base, size);
        Fr cur = tile_scan<Op, SCAN_K, true>(x, pw, run, sh + (i & 1) * SCAN_WAVES * 32);
#pragma unroll
        for (int k = 0; k < SCAN_K; ++k) {
            const int kk = Op::REV ? SCAN_K - 1 - k : k;
            if constexpr (INCLUSIVE) cur = Op::step(cur, x[kk], pw.unit);
            if (base + kk < size) store<FrCfg>(out + 32 * (base + kk), cur);
            if constexpr (!INCLUSIVE) cur = Op::step(cur, x[kk], pw.unit);
        }
    }
}

// ---- host side
struct ScanCall {
    size_t size;
    uint32_t batch;
    ScanGeom g;
};
// the checks every scan entry shares, before any device work
static eIcicleError scan_call(size_t size, const VecOpsConfig* cfg, ScanCall* c) {
    if (cfg->columns_batch) return MBLS_API_NOT_IMPLEMENTED;
    const size_t batch = cfg->batch_size > 0 ? (size_t)cfg->batch_size : 1;
    if (size == 0 || size > SCAN_MAX_ELEMS || size * batch > SCAN_MAX_ELEMS) return MBLS_INVALID_ARGUMENT;
    c->size = size;
    c->batch = (uint32_t)batch;
    c->g = scan_geom(size);
    return MBLS_SUCCESS;
}

// the three launches over device operands; out null: launches 1 and 2 only
template <class Op, bool INCLUSIVE>
static eIcicleError scan_launch(const ScanCall& c, uint8_t* out, const uint8_t* in, const uint8_t* zs, const uint8_t* init,
                                uint8_t* total, uint8_t* agg, uint8_t* carry, hipStream_t st) {
    const dim3 grid(c.batch * c.g.groups), block(SCAN_THREADS);
    hipLaunchKernelGGL(k_scan_reduce<Op>, grid, block, 0, st, agg, in, zs, c.size, c.g);
    hipLaunchKernelGGL(k_scan_aggregates<Op>, dim3(c.batch), block, 0, st, out ? carry : nullptr, total, agg, zs, init,
                       c.g);
    if (out) hipLaunchKernelGGL((k_scan_write<Op, INCLUSIVE>), grid, block, 0, st, out, in, carry, zs, c.size, c.g);
    MBLS_TRY(hipGetLastError());
    return MBLS_SUCCESS;
}

}  // namespace mbls
