// mbls_sort.hpp -- what the Fr column sort (sort.hip) shares with the log-derivative lookup's join
// (logup.hip): the geometry, the scratch layout, the key helpers and the sort itself.
#pragma once
#include <hip/hip_runtime.h>

#include "mbls_common.hpp"
#include "mbls_field.hpp"

namespace mbls {

// ---- geometry: the constants live here and nowhere else (mbls_fr_sort_plan reports them)
#ifndef MBLS_SORT_SKIP
#define MBLS_SORT_SKIP 1  // 0: no uniform-word flags (A/B builds only)
#endif
static constexpr bool SORT_SKIP = MBLS_SORT_SKIP != 0;
static constexpr int SORT_BITS = 8;
static constexpr int SORT_DIGITS = 1 << SORT_BITS;
static constexpr int SORT_THREADS = 256;
static constexpr int SORT_WAVE = 64;
static constexpr int SORT_WAVES = SORT_THREADS / SORT_WAVE;
static constexpr int SORT_K = 8;                          // rounds per tile (scatter), entries per thread (rank scan)
static constexpr int SORT_TILE = SORT_K * SORT_THREADS;   // elements per workgroup tile
static constexpr int SORT_SUMS_K = 2;                     // table entries per thread in the one-workgroup scans
static constexpr int SORT_MAX_GROUPS = SORT_SUMS_K * SORT_THREADS;
static constexpr int SORT_KEY_WORDS = 8;
static constexpr int SORT_WORD_PASSES = 32 / SORT_BITS;
static constexpr size_t SORT_MAX_ELEMS = (size_t)1 << 26;
static_assert(SORT_DIGITS == SORT_THREADS, "one thread per digit in the tables");
static_assert(SORT_WORD_PASSES % 2 == 0, "a word's passes end in the buffer they began in");

struct SortGeom {
    uint32_t n;       // elements of all members together (the lookup: inputs then tables)
    uint32_t span;    // elements per workgroup: tiles_per_group * SORT_TILE
    uint32_t groups;  // workgroups per pass, <= SORT_MAX_GROUPS
};
static SortGeom sort_geom(size_t n) {
    const size_t tiles = (n + SORT_TILE - 1) / SORT_TILE;
    size_t per = (tiles + SORT_MAX_GROUPS - 1) / SORT_MAX_GROUPS;
    if (per == 0) per = 1;
    SortGeom g;
    g.n = (uint32_t)n;
    g.span = (uint32_t)(per * SORT_TILE);
    g.groups = (uint32_t)((n + g.span - 1) / g.span);
    if (g.groups == 0) g.groups = 1;
    return g;
}
// stable passes over the member number: 8-bit digits of members - 1
static int sort_member_passes(size_t members) {
    int p = 0;
    for (size_t top = members - 1; top; top >>= SORT_BITS) ++p;
    return p;
}

// control words, zeroed by one memset per call
static constexpr int SORT_MAX_PASSES = SORT_KEY_WORDS * SORT_WORD_PASSES + 4;
static constexpr size_t SORT_CTL_VARIES = (size_t)SORT_MAX_PASSES * SORT_DIGITS;  // after the digit totals
static constexpr size_t SORT_CTL_WORDS = SORT_CTL_VARIES + SORT_KEY_WORDS + 1;

// the scratch block of one call, single-sourced for the entries and mbls_fr_sort_plan
struct SortLayout {
    size_t planes, word_a, idx_a, word_b, idx_b, hist, ctl;  // the sort
    size_t tsorted, flags, sums, left, missing;              // the lookup (keys alias planes)
    size_t bytes;
};
static SortLayout sort_layout(size_t n, bool lookup, size_t batch) {
    SortLayout L{};
    // the table's rows are sized by the tile count, capped: it never shrinks as n grows, though
    // the workgroup count does where a span gets another tile
    const size_t tiles = (n + SORT_TILE - 1) / SORT_TILE;
    const size_t groups = tiles < (size_t)SORT_MAX_GROUPS ? tiles : (size_t)SORT_MAX_GROUPS;
    size_t at = 0;
    auto put = [&](size_t bytes) {
        const size_t p = at;
        at += align_up(bytes);
        return p;
    };
    L.planes = put(32 * n);
    L.word_a = put(4 * n);
    L.idx_a = put(4 * n);
    L.word_b = put(4 * n);
    L.idx_b = put(4 * n);
    L.hist = put(4 * (size_t)SORT_DIGITS * groups);
    L.ctl = put(4 * SORT_CTL_WORDS);
    if (lookup) {
        L.tsorted = put(32 * (n / 2));
        L.flags = put(4 * (n + 1));
        L.sums = put(4 * (size_t)SORT_MAX_GROUPS);
        L.left = put(4 * (n / 2));
        L.missing = put(8 * batch);
    }
    L.bytes = at;
    return L;
}

// ---- device helpers
// the lanes of this wave that hold the same low `bits` bits of v as this one (valid lanes only);
// bits is the same in every lane
MBLS_DEV uint64_t match_bits(uint32_t v, bool valid, int bits) {
    uint64_t peers = __ballot(valid);
    for (int b = 0; b < bits; ++b) {
        const bool bit = (v >> b) & 1;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}
// the lanes of this wave that hold the same digit as this one (valid lanes only)
MBLS_DEV uint64_t match_digit(uint32_t d, bool valid) {
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < SORT_BITS; ++b) {
        const bool bit = (d >> b) & 1;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

MBLS_DEV bool key_less(const Fr& a, const Fr& b) {
    bool lt = false, eq = true;
#pragma unroll
    for (int w = SORT_KEY_WORDS - 1; w >= 0; --w) {
        lt = lt || (eq && a.v[w] < b.v[w]);
        eq = eq && a.v[w] == b.v[w];
    }
    return lt;
}

MBLS_DEV Fr sort_key(const Fr& x, bool mont) { return mont ? from_mont(x) : x; }

// ---- host side
static unsigned sort_blocks(size_t n) { return (unsigned)((n + SORT_THREADS - 1) / SORT_THREADS); }

struct SortCall {
    size_t size, batch;
};
static eIcicleError sort_call(size_t size, const VecOpsConfig* cfg, SortCall* c) {
    if (cfg->columns_batch) return MBLS_API_NOT_IMPLEMENTED;
    const size_t batch = cfg->batch_size > 0 ? (size_t)cfg->batch_size : 1;
    if (size == 0 || size > SORT_MAX_ELEMS || size * batch > SORT_MAX_ELEMS) return MBLS_INVALID_ARGUMENT;
    c->size = size;
    c->batch = batch;
    return MBLS_SUCCESS;
}

// Sorts the g.n elements src0[0 .. n0) ++ src1[0 .. n - n0), members of `size`; returns the buffer
// holding the sorted permutation (global indices) in *idx_out.  `scratch` holds L.bytes; the key
// planes stay as written until the caller reuses them.  Defined in sort.hip.
eIcicleError sort_launch(const SortGeom& g, size_t size, uint8_t* scratch, const SortLayout& L, const uint8_t* src0,
                         const uint8_t* src1, uint32_t n0, bool mont, hipStream_t st, const uint32_t** idx_out);

}  // namespace mbls
