// mbls_fixed_base.hpp -- geometry and digit recoding of the fixed-base multiplication
// (fixed_base.hip), as host-and-device code: the kernels and the host probe
// (mbls_fixed_base_recode) run the same function.  No HIP is needed to include this file.
//
// k < r is written in signed radix 2^c, k = sum_w d_w 2^(c w), w < W = ceil(255 / c): window w is
// the c bits of k from bit c w on, plus the carry of the window below; a value >= 2^(c-1) becomes
// value - 2^c with a carry of one into the next window.  So d_w lies in [-2^(c-1), 2^(c-1) - 1],
// except in the top window, which keeps its carry and stays non-negative: r < 2^255 leaves it at
// most 255 - c (W - 1) bits, so d_(W-1) <= 2^(255 - c (W-1)) - 1 + 1 <= 2^(c-1) (at c = 12:
// r >> 252 = 7, so d_21 <= 8; at c = 8: r >> 248 = 0x73, so d_31 <= 0x74).  The table
// therefore holds |d| = 1 .. 2^(c-1) per window.
// The digits come out lowest window first and the scalar is consumed by shifting, so that a kernel
// needs neither a digit array nor a run-time index into the scalar's words.
#pragma once
#include <stdint.h>

#ifndef MBLS_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MBLS_HD __host__ __device__ __forceinline__
#else
#define MBLS_HD inline
#endif
#endif

namespace mbls {
namespace fb {

constexpr int C = 12;                     // digit width, G1 and G2 (measured against 8 and 10: DESIGN.md 5.16)
constexpr int WINDOWS = (255 + C - 1) / C;  // r < 2^255
constexpr int ROWS = 1 << (C - 1);        // table entries per window: |d| = 1 .. 2^(c-1)
constexpr int ENTRIES = WINDOWS * ROWS;
constexpr int BLOCK = 64;                 // one wave per workgroup: no LDS, no barrier
constexpr int MAX_BATCH = 1 << 26;
// lanes per launch: bounds the Jacobian work array (G1 144 MiB, G2 72 MiB) whatever the batch size
constexpr int G1_CHUNK = 1 << 20;
constexpr int G2_CHUNK = 1 << 18;

static_assert(C >= 2 && C <= 16, "a digit is taken from the low word");
static_assert((WINDOWS - 1) * C < 255, "the top window is not empty");
static_assert(255 - (WINDOWS - 1) * C <= C - 1, "the top digit with its carry stays within the table");

// r, little-endian 32-bit words
MBLS_HD uint32_t modulus_word(int i) {
    constexpr uint32_t R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                               0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
    return R[i];
}

// k mod r for any 256-bit k: 2^256 < 3r, two conditional subtractions (the reduction of
// mbls_split.hpp's reduce_scalar_words, restated so that the host can run it)
MBLS_HD void reduce(uint32_t (&k)[8]) {
    for (int rep = 0; rep < 2; ++rep) {
        uint32_t t[8];
        uint64_t br = 0;
        for (int i = 0; i < 8; ++i) {
            const uint64_t d = (uint64_t)k[i] - modulus_word(i) - br;
            t[i] = (uint32_t)d;
            br = (d >> 63) & 1;
        }
        for (int i = 0; i < 8; ++i) k[i] = br ? k[i] : t[i];
    }
}

// the digit of the lowest window still in k; k >>= c.  `carry` starts at 0 and is carried from call
// to call; `top` marks window W - 1, which keeps its carry
MBLS_HD int next_digit(uint32_t (&k)[8], uint32_t& carry, bool top) {
    const uint32_t raw = (k[0] & ((1u << C) - 1)) + carry;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int i = 0; i < 7; ++i) k[i] = (k[i] >> C) | (k[i + 1] << (32 - C));
    k[7] >>= C;
    if (!top && raw >= (1u << (C - 1))) {
        carry = 1;
        return (int)raw - (1 << C);
    }
    carry = 0;
    return (int)raw;
}

// all W digits of k < r, lowest window first (the host probe and the models' comparison)
MBLS_HD void recode(const uint32_t (&k_in)[8], int32_t (&digits)[WINDOWS]) {
    uint32_t k[8], carry = 0;
    for (int i = 0; i < 8; ++i) k[i] = k_in[i];
    for (int w = 0; w < WINDOWS; ++w) digits[w] = next_digit(k, carry, w == WINDOWS - 1);
}

// the table row of digit d != 0 in window w: entry [|d| 2^(c w)] base
MBLS_HD uint32_t table_index(int w, int d) { return (uint32_t)w * ROWS + (uint32_t)((d < 0 ? -d : d) - 1); }

}  // namespace fb
}  // namespace mbls
