// serde.hip -- batch compression and decompression of G1 / G2 points in the ZCash encoding that
// ceremony transcripts, SRS files and the blst-backed crates' to_compressed / from_compressed use.
// (No reference counterpart: the reference has no serialization and no square root.)
//
// Format.  G1: 48 bytes, x as a big-endian integer; G2: 96 bytes, x.c1 then x.c0.  The top three
// bits of byte 0 are flags: C (bit 7) compressed form, always set; I (bit 6) infinity, then every
// other bit is zero; S (bit 5) y is the larger of {y, -y} as standard-form integers, for G2 comparing
// c1 first and c0 only when y.c1 == 0.
//
// One lane per G1 point, a pair of lanes per G2 point (lane j holds component j of every Fq2
// value, mbls_pairfield.hpp), one wave per workgroup, no LDS, no table in memory.  Records move as
// 16-byte vectors and are byte-swapped in registers.  Decompression, in the order of
// mbls_decode_status: the flags on the raw top word, the infinity encoding, x < p on the raw words,
// then y = sqrt(x^3 + b) by the fixed exponent chain of mbls_sqrt.hpp (the only expensive part: one
// chain per G1 point, two per G2 pair) and the choice between y and -y on standard-form words.  A
// lane that fails a test leaves with its status and an all-zero point; the chain's steps are the
// same for every lane, so a wave diverges only at those exits (and, in G2, around the norm's root
// for the pairs whose radicand is real).  No subgroup test: mbls_g*_check_points composes.
// Compression is the memory-bound inverse and validates nothing.
// Not constant time (nothing secret is involved).
#include <hip/hip_runtime.h>

#include "mbls_common.hpp"
#include "mbls_curve.hpp"
#include "mbls_scalar_mul.hpp"
#include "mbls_sqrt.hpp"

namespace mbls {

static constexpr int SD_MAX_BATCH = 1 << 26;  // scalar_mul's bound (SM_MAX_BATCH)
static constexpr uint32_t SD_LANES_G2 = LaneOf<Fq2>::LANES;
static constexpr uint32_t FLAG_C = 4, FLAG_I = 2, FLAG_S = 1;  // the top word >> 29

// 48 big-endian bytes <-> 12 little-endian words: word 11 - k is the byte-swapped k-th word in memory
MBLS_DEV Fq sd_load_be(const uint8_t* p) {
    Fq r;
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const uint4 x = q[i];
        r.v[11 - 4 * i] = __builtin_bswap32(x.x);
        r.v[10 - 4 * i] = __builtin_bswap32(x.y);
        r.v[9 - 4 * i] = __builtin_bswap32(x.z);
        r.v[8 - 4 * i] = __builtin_bswap32(x.w);
    }
    return r;
}
MBLS_DEV void sd_store_be(uint8_t* p, const Fq& a) {
    uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
    for (int i = 0; i < 3; ++i)
        q[i] = make_uint4(__builtin_bswap32(a.v[11 - 4 * i]), __builtin_bswap32(a.v[10 - 4 * i]),
                          __builtin_bswap32(a.v[9 - 4 * i]), __builtin_bswap32(a.v[8 - 4 * i]));
}
// raw words < p (sub_mod_raw borrows exactly then)
MBLS_DEV bool sd_canonical(const Fq& a) {
    uint32_t t[12];
    return sub_mod_raw<FqCfg>(t, a.v) != 0;
}
MBLS_DEV Fq sd_four() { return dbl(dbl(Fq::one())); }

// the S rule on a pair's standard-form y: c1 decides, c0 only when y.c1 == 0 (on both lanes; every
// exchange runs before the choice)
MBLS_DEV bool sd_pair_larger(const Fq& y) {
    const bool big = fsqrt::is_larger_half(y);
    const bool big0 = fsqrt::pair_even(big), big1 = fsqrt::pair_odd(big), zero1 = fsqrt::pair_odd(y.is_zero());
    return zero1 ? big0 : big1;
}

// Writes point i (all-zero unless the status is OK) and returns its status.
template <bool MONT>
MBLS_DEV uint8_t decompress_g1(const uint8_t* __restrict__ bytes, uint8_t* __restrict__ points, uint32_t i) {
    Affine<Fq> out = Affine<Fq>::inf();
    uint8_t st = MBLS_DECODE_OK;
    Fq x = sd_load_be(bytes + (size_t)i * 48);
    const uint32_t flags = x.v[11] >> 29;
    x.v[11] &= 0x1fffffffu;
    if (!(flags & FLAG_C) || ((flags & FLAG_I) && ((flags & FLAG_S) || !x.is_zero()))) {
        st = MBLS_DECODE_BAD_FLAGS;
    } else if (flags & FLAG_I) {
        st = MBLS_DECODE_IDENTITY;
    } else if (!sd_canonical(x)) {
        st = MBLS_DECODE_NONCANONICAL;
    } else {
        const Fq xm = to_mont(x);
        Fq y, t;
        if (!fsqrt::root(y, t, sqr(xm) * xm + sd_four())) {
            st = MBLS_DECODE_NO_POINT;
        } else {
            // the sign on standard-form words; negation is the same operation in either form
            const Fq ys = from_mont(y);
            const bool flip = fsqrt::is_larger_half(ys) != ((flags & FLAG_S) != 0);
            out.x = MONT ? xm : x;
            out.y = MONT ? y : ys;
            if (flip) out.y = neg(out.y);
        }
    }
    store_affine<Fq>(points, i, out);
    return st;
}

// G2: both lanes of a pair call this with the same i; the odd lane reads x.c1 (bytes 0..47, with
// the flags), the even lane x.c0 (bytes 48..95).  Every predicate is combined over the pair.
template <bool MONT>
MBLS_DEV uint8_t decompress_g2(const uint8_t* __restrict__ bytes, uint8_t* __restrict__ points, uint32_t i) {
    const bool odd = pairdpp::odd();
    Affine<PFq2> out = Affine<PFq2>::inf();
    uint8_t st = MBLS_DECODE_OK;
    PFq2 x{sd_load_be(bytes + (size_t)i * 96 + (odd ? 0 : 48))};
    const uint32_t top = x.v.v[11] >> 29;
    const uint32_t flags = fsqrt::pair_odd(top);  // the even lane's top bits belong to x.c0
    if (odd) x.v.v[11] &= 0x1fffffffu;
    if (!(flags & FLAG_C) || ((flags & FLAG_I) && ((flags & FLAG_S) || !x.is_zero()))) {
        st = MBLS_DECODE_BAD_FLAGS;
    } else if (flags & FLAG_I) {
        st = MBLS_DECODE_IDENTITY;
    } else if (!fsqrt::pair_all(sd_canonical(x.v))) {
        st = MBLS_DECODE_NONCANONICAL;
    } else {
        const PFq2 xm{to_mont(x.v)};
        PFq2 y;
        if (!fsqrt::root(y, sqr(xm) * xm + PFq2{sd_four()})) {  // b = 4 + 4 u
            st = MBLS_DECODE_NO_POINT;
        } else {
            const Fq ys = from_mont(y.v);
            const bool larger = sd_pair_larger(ys);
            out.x = MONT ? xm : x;
            out.y.v = MONT ? y.v : ys;
            if (larger != ((flags & FLAG_S) != 0)) out.y = neg(out.y);
        }
    }
    store_affine<PFq2>(points, i, out);
    return st;
}

// status may be null.  Lane t works on record t / LANES (G2: whole pairs, so lanes past n leave in
// pairs); the first lane of a point reports it.  Every lane of the wave reaches the ballot: lanes
// past n vote valid; lane 0 adds the wave's count with one ordinary atomic.
template <bool G2, bool MONT>
__global__ __launch_bounds__(SM_BLOCK) void k_decompress(const uint8_t* __restrict__ bytes, uint8_t* __restrict__ points,
                                                         uint8_t* __restrict__ status,
                                                         unsigned long long* __restrict__ n_invalid, uint32_t n) {
    constexpr uint32_t LANES = G2 ? SD_LANES_G2 : 1;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = t / LANES;
    const bool first = t % LANES == 0;
    uint8_t s = MBLS_DECODE_OK;
    if (i < n) {
        if constexpr (G2)
            s = decompress_g2<MONT>(bytes, points, i);
        else
            s = decompress_g1<MONT>(bytes, points, i);
        if (status && first) status[i] = s;
    }
    const unsigned long long bad = __ballot(first && s >= MBLS_DECODE_NONCANONICAL);
    if (threadIdx.x == 0 && bad) atomicAdd(n_invalid, (unsigned long long)__popcll(bad));
}

// Compression: the all-zero identity gives c0 00 .. 00; nothing is validated.
template <bool G2, bool MONT>
__global__ __launch_bounds__(SM_BLOCK) void k_compress(const uint8_t* __restrict__ points, uint8_t* __restrict__ bytes,
                                                       uint32_t n) {
    constexpr uint32_t LANES = G2 ? SD_LANES_G2 : 1;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = t / LANES;
    if (i >= n) return;
    if constexpr (G2) {
        const bool odd = pairdpp::odd();
        const Affine<PFq2> b = load_affine<PFq2>(points, i);
        const bool inf = b.is_inf();
        Fq x = MONT ? from_mont(b.x.v) : b.x.v;
        const Fq y = MONT ? from_mont(b.y.v) : b.y.v;
        const bool larger = sd_pair_larger(y);
        if (odd) x.v[11] |= (FLAG_C | (inf ? FLAG_I : 0u) | (larger ? FLAG_S : 0u)) << 29;
        sd_store_be(bytes + (size_t)i * 96 + (odd ? 0 : 48), x);
    } else {
        const Affine<Fq> b = load_affine<Fq>(points, i);
        const bool inf = b.is_inf();
        Fq x = MONT ? from_mont(b.x) : b.x;
        const Fq y = MONT ? from_mont(b.y) : b.y;
        x.v[11] |= (FLAG_C | (inf ? FLAG_I : 0u) | (fsqrt::is_larger_half(y) ? FLAG_S : 0u)) << 29;
        sd_store_be(bytes + (size_t)i * 48, x);
    }
}

// a device operand moves as 16-byte vectors; a host one is staged into the (256-byte aligned) arena
static bool sd_misaligned(const void* p, bool on_device) { return on_device && ((uintptr_t)p & 15) != 0; }

template <bool G2>
static eIcicleError decompress_call(const uint8_t* bytes, int size, bool mont, const VecOpsConfig* cfg, void* points,
                                    uint8_t* status, uint64_t* n_invalid) {
    if (!bytes || !cfg || !points) return MBLS_INVALID_ARGUMENT;
    if (size <= 0 || size > SD_MAX_BATCH) return MBLS_INVALID_ARGUMENT;
    if (sd_misaligned(bytes, cfg->is_a_on_device) || sd_misaligned(points, cfg->is_result_on_device))
        return MBLS_INVALID_ARGUMENT;
    constexpr size_t AFF = PointSize<typename std::conditional<G2, Fq2, Fq>::type>::AFF, REC = AFF / 2;
    const size_t n = (size_t)size;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    Staging S(st, Staging::LEASE_ALWAYS);
    uint8_t *cnt, *dpts, *dst = nullptr;
    const uint8_t* db;
    S.scratch(&cnt, sizeof(unsigned long long));
    S.in(&db, bytes, n * REC, cfg->is_a_on_device);
    S.out(&dpts, points, n * AFF, cfg->is_result_on_device);
    if (status) S.out(&dst, status, n, cfg->is_result_on_device);
    const eIcicleError er = S.open();
    if (er != MBLS_SUCCESS) return er;
    MBLS_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), st));
    {
        ProfScope prof(G2 ? "serde.decompress.g2" : "serde.decompress.g1", st);
        const uint32_t lanes = (uint32_t)n * (G2 ? SD_LANES_G2 : 1);  // <= 2^27
        const dim3 grid((lanes + SM_BLOCK - 1) / SM_BLOCK), block(SM_BLOCK);
        unsigned long long* dc = reinterpret_cast<unsigned long long*>(cnt);
        if (mont)
            hipLaunchKernelGGL((k_decompress<G2, true>), grid, block, 0, st, db, dpts, dst, dc, (uint32_t)n);
        else
            hipLaunchKernelGGL((k_decompress<G2, false>), grid, block, 0, st, db, dpts, dst, dc, (uint32_t)n);
        MBLS_TRY(hipGetLastError());
    }
    // the count is a host output: it makes the call synchronous, as a host buffer does
    if (n_invalid) MBLS_TRY(hipMemcpyAsync(n_invalid, cnt, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    return S.close(cfg->is_async && !n_invalid);
}

template <bool G2>
static eIcicleError compress_call(const void* points, int size, bool mont, const VecOpsConfig* cfg, uint8_t* bytes) {
    if (!points || !cfg || !bytes) return MBLS_INVALID_ARGUMENT;
    if (size <= 0 || size > SD_MAX_BATCH) return MBLS_INVALID_ARGUMENT;
    if (sd_misaligned(points, cfg->is_a_on_device) || sd_misaligned(bytes, cfg->is_result_on_device))
        return MBLS_INVALID_ARGUMENT;
    constexpr size_t AFF = PointSize<typename std::conditional<G2, Fq2, Fq>::type>::AFF, REC = AFF / 2;
    const size_t n = (size_t)size;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    Staging S(st, Staging::LEASE_IF_STAGED);
    uint8_t* db;
    const uint8_t* dp;
    S.in(&dp, points, n * AFF, cfg->is_a_on_device);
    S.out(&db, bytes, n * REC, cfg->is_result_on_device);
    const eIcicleError er = S.open();
    if (er != MBLS_SUCCESS) return er;
    {
        ProfScope prof(G2 ? "serde.compress.g2" : "serde.compress.g1", st);
        const uint32_t lanes = (uint32_t)n * (G2 ? SD_LANES_G2 : 1);  // <= 2^27
        const dim3 grid((lanes + SM_BLOCK - 1) / SM_BLOCK), block(SM_BLOCK);
        if (mont)
            hipLaunchKernelGGL((k_compress<G2, true>), grid, block, 0, st, dp, db, (uint32_t)n);
        else
            hipLaunchKernelGGL((k_compress<G2, false>), grid, block, 0, st, dp, db, (uint32_t)n);
        MBLS_TRY(hipGetLastError());
    }
    return S.close(cfg->is_async);
}

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError mbls_g1_decompress(const uint8_t* bytes, int size, bool points_montgomery, const VecOpsConfig* config,
                                mbls_g1_affine_t* points, uint8_t* status, uint64_t* n_invalid) {
    return decompress_call<false>(bytes, size, points_montgomery, config, points, status, n_invalid);
}
eIcicleError mbls_g2_decompress(const uint8_t* bytes, int size, bool points_montgomery, const VecOpsConfig* config,
                                mbls_g2_affine_t* points, uint8_t* status, uint64_t* n_invalid) {
    return decompress_call<true>(bytes, size, points_montgomery, config, points, status, n_invalid);
}
eIcicleError mbls_g1_compress(const mbls_g1_affine_t* points, int size, bool points_montgomery,
                              const VecOpsConfig* config, uint8_t* bytes) {
    return compress_call<false>(points, size, points_montgomery, config, bytes);
}
eIcicleError mbls_g2_compress(const mbls_g2_affine_t* points, int size, bool points_montgomery,
                              const VecOpsConfig* config, uint8_t* bytes) {
    return compress_call<true>(points, size, points_montgomery, config, bytes);
}

}  // extern "C"
