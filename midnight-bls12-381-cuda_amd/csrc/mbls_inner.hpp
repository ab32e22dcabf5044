// mbls_inner.hpp -- host-only geometry of the Fr inner products (inner.hip): the tile, the blocking
// of columns and vectors, the row groups and the scratch layout.  One function decides them for the
// launches and for mbls_fr_inner_plan, so the tests read the numbers the kernels run with.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mbls {

static constexpr int INNER_THREADS = 256;
// products a thread adds into its unreduced 64-bit columns before one Montgomery reduction: the
// rows it takes from one tile.  Bound: see inner.hip (7 * 9 * 2^58 < 2^64)
static constexpr int INNER_DEFER = 7;
static constexpr int INNER_TILE = INNER_THREADS * INNER_DEFER;  // rows per tile
static constexpr int INNER_CB = 2;                              // columns per block
static constexpr int INNER_VB = 2;                              // vectors per block
static constexpr uint32_t INNER_TARGET_WGS = 4096;  // workgroups aimed at over all blocks
static constexpr uint32_t INNER_MAX_GROUPS = 1024;  // row groups per block, at the most
static constexpr size_t INNER_MAX_ROWS = (size_t)1 << 26;
static constexpr int INNER_MAX_COLUMNS = 1024;
static constexpr int INNER_MAX_VECTORS = 16;

static inline size_t inner_align(size_t x) { return (x + 255) / 256 * 256; }

struct InnerGeom {
    uint32_t ncb, nvb;          // column blocks, vector blocks
    uint32_t tiles;             // tiles of the rows
    uint32_t group_cap;         // most row groups this (n_columns, n_vectors) may take
    uint32_t tiles_per_group;   // consecutive tiles one workgroup sums
    uint32_t groups;            // row groups: partial sums per output
    size_t partial_bytes;       // 32 * groups * n_columns * n_vectors, rounded to 256
    size_t table_bytes;         // the device copy of the two pointer tables, rounded to 256
    int pow_log;                // s of base^i = hi[i >> s] * lo[i & (2^s - 1)]
    size_t pow_lo, pow_hi;      // entries of the two tables per member
};

// s = ceil(log2(size) / 2): both tables hold about sqrt(size) entries
static inline int inner_pow_log(size_t size) {
    int lg = 0;
    while (((size_t)1 << lg) < size) ++lg;
    return (lg + 1) / 2;
}

static inline InnerGeom inner_geom(size_t size, int n_columns, int n_vectors) {
    InnerGeom g;
    g.ncb = (uint32_t)((n_columns + INNER_CB - 1) / INNER_CB);
    g.nvb = (uint32_t)((n_vectors + INNER_VB - 1) / INNER_VB);
    g.tiles = (uint32_t)((size + INNER_TILE - 1) / INNER_TILE);
    const uint32_t blocks = g.ncb * g.nvb;
    g.group_cap = INNER_TARGET_WGS / blocks;
    if (g.group_cap < 1) g.group_cap = 1;
    if (g.group_cap > INNER_MAX_GROUPS) g.group_cap = INNER_MAX_GROUPS;
    g.tiles_per_group = (g.tiles + g.group_cap - 1) / g.group_cap;
    g.groups = (g.tiles + g.tiles_per_group - 1) / g.tiles_per_group;
    g.partial_bytes = inner_align((size_t)32 * g.groups * (size_t)n_columns * (size_t)n_vectors);
    g.table_bytes = inner_align(sizeof(void*) * (size_t)(n_columns + n_vectors));
    g.pow_log = inner_pow_log(size);
    g.pow_lo = (size_t)1 << g.pow_log;
    g.pow_hi = (size + g.pow_lo - 1) >> g.pow_log;
    return g;
}

// scratch of mbls_fr_powers for `batch` members (also the tables multi_eval builds)
static inline size_t inner_pow_table_bytes(const InnerGeom& g, size_t batch) {
    return inner_align((size_t)32 * batch * (g.pow_lo + g.pow_hi));
}

}  // namespace mbls
