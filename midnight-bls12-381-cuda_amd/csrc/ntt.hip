// ntt.hip -- radix-2 Fr NTT for CDNA4 (natural-order core; orderings / columns_batch by permutation).
//
// Semantics = the CPU path the prover uses (core/ntt.rs:1488-1603, midnight_curves best_fft):
//   forward  X_j = sum_i x_i w^(ij),  inverse  x_i = n^-1 sum_j X_j w^(-ij),
//   w = ROOT_OF_UNITY^(2^(32-k)) for n = 2^k, ROOT_OF_UNITY = 7^((r-1)/2^32).
// The reference GPU NTT (ntt_kernels.cu:710-958) derives its twiddles from whatever root the
// caller passes assuming order 2^24 (ntt_kernels.cu:1614,1644) and does not match best_fft
// (SURVEY.md finding 2); we do not reproduce that.
//
// Data layout in HBM: n contiguous 32-byte Fr values per polynomial, batch polynomials
// back to back (other layouts are permuted in and out).  Twiddles: per-stage tables
// concatenated, stage s (m = 2^s) holding w_(2^s)^i, i < 2^(s-1), at offset 2^(s-1) - 1
// (2^L - 1 entries for stages 1..L), so adjacent columns of a tile read adjacent twiddles.
// Each entry is w R' mod r in radix-2^29 limbs (mbls_fr29.hpp: the butterflies' products run in
// that form), stored as three planes -- limbs 0-3 (16 B), limbs 4-7 (16 B), limb 8 (4 B) -- so
// every twiddle is three aligned loads (36 B per entry).
// (A single w_(2^K)^i table read at stride 2^(K-s) put every lane on its own cache line:
// measured 3.5x the data bytes fetched by the later passes, profiles/r01.)
//
// Kernel structure: ceil(k / MBLS_NTT_PASS_STAGES) = ceil(k / 8) passes of near-equal stage
// counts (pass_plan: the one plan every transform here runs and mbls_fr_domain_plan reports), each
// a LDS-resident tile of T = 2^MBLS_NTT_TILE_LOG = 1024 elements (32 KiB) doing up to 8 radix-2
// DIT stages (2^L rows x 2^(10 - L) adjacent columns) between __syncthreads.
// A pass kernel is a load phase, the stage engine, and a store:
//   tile_stages  the engine, once: the radix-4 stage pairs, the radix-2 tail and the store of a tile
//                with no stage left, over a tile in LDS, from any first stage; it hands every
//                finished value to the kernel's put(row, col, v).  The lazy [0, 2r) range argument,
//                the twiddle indexing and the barrier placement live there and nowhere else.
//   k_ntt_pass   the plain transform.  Load: pass 1 fuses the bit-reversal permutation into its
//                gather (C adjacent columns of the input viewed as a 2^L x 2^(k-L) matrix, coalesced
//                C*32-byte rows, written back as contiguous DIT blocks); later passes read and write
//                tiles of 2^L strided rows x C adjacent columns in place.  put: the last pass stores
//                canonical values, the inverse's multiplied by n^-1.  All stages, from l = 1.
//   k_dom_pass   the first and last passes of the extended-coset transforms of a halo2-style
//                EvaluationDomain (mbls_fr_coeff_to_extended, mbls_fr_extended_to_coeff; the domain
//                section at the end of the file).  Load: zero padding, coset scaling and the rows
//                that stages 1..Ee would only copy, or the vanishing table.  put: the inverse coset
//                product and the truncated store.  Stages from l = Ee + 1; the passes between its
//                first and last are k_ntt_pass as it stands.
// Algorithmic traffic: 64 B per element per transform (one read + one write of 32 B);
// actual traffic = passes * 64 B + twiddle reads.  Arithmetic: (n/2) log n Montgomery
// products -- the kernel is VALU-bound on gfx950.
#include <hip/hip_runtime.h>
#include <string.h>

#include <memory>
#include <mutex>
#include <vector>

#include "mbls_common.hpp"
#include "mbls_field.hpp"
#include "mbls_fr29.hpp"

namespace mbls {

#ifndef MBLS_NTT_TILE_LOG
#define MBLS_NTT_TILE_LOG 10
#endif
#ifndef MBLS_NTT_PASS_STAGES
#define MBLS_NTT_PASS_STAGES 8
#endif
#ifndef MBLS_NTT_THREADS
#define MBLS_NTT_THREADS 256
#endif
static constexpr int NTT_TILE_LOG = MBLS_NTT_TILE_LOG;
static constexpr int NTT_TILE = 1 << NTT_TILE_LOG;  // elements per workgroup tile
static constexpr int NTT_THREADS = MBLS_NTT_THREADS;
static constexpr int NTT_PASS_STAGES = MBLS_NTT_PASS_STAGES;

// canonical 2^32-th root of unity, Montgomery (bls12_381_constants.h:127-130)
static const uint64_t ROOT_2_32_MONT[4] = {0xb9b58d8c5f0e466aULL, 0x5b1b4c801819d7ecULL, 0x0af53ae352a31e64ULL,
                                           0x5bf3adda19e9b27bULL};

// the end of a table set (DomainTables, CosetTables): wait for the device that owns it, then free
static void sync_and_free(int device, void* a, void* b = nullptr) {
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != device) (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();  // every transform that read the tables has finished
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (cur != device) (void)hipSetDevice(cur);
}

// Twiddle tables of one domain build.  Callers take a shared_ptr snapshot under the lock and
// enqueue their kernels with it; a table superseded by an extension or a release is freed only
// when the last snapshot is dropped, and then only after a device synchronisation -- no queued
// transform ever reads freed memory (concurrent callers on rayon threads, SURVEY.md 8b
// "Threading").  Release / extension happen once per domain size, so the synchronisation is
// rare; an event recorded after every transform instead (round 3) cost ~5 us of dispatch delay
// per transform (an event marker holds the next dispatch: profiles/r04/gapbench_markers.txt).
struct DomainTables {
    int max_log = 0;            // stage tables built for stages 1..max_log
    uint32_t count = 0;         // entries per table (2^max_log - 1): the limb planes' stride
    int device = 0;             // device the tables live on
    uint8_t* tw = nullptr;      // per-stage w_(2^s)^i tables (see header)
    uint8_t* tw_inv = nullptr;  // per-stage w_(2^s)^-i
    ~DomainTables() { sync_and_free(device, tw, tw_inv); }
};

// Coset power tables of the extended-coset transforms (see the domain section below): built once
// per (generator, size, direction) and cached in the device's domain, with the same lifetime rule
// as DomainTables -- a caller enqueues with a shared_ptr snapshot, and the memory is freed after a
// device synchronisation when the last snapshot is dropped.
struct CosetTables {
    int device = 0;
    uint64_t g[4] = {0, 0, 0, 0};  // the caller's generator (Montgomery), the cache key with:
    int log_n = 0, sh = 0;         // transform size and index split i = ((i >> sh) << sh) + (i & (2^sh - 1))
    bool inverse = false;
    uint8_t* mem = nullptr;        // A (2^(log_n - sh) entries) then B (2^sh entries), 32 B each
    const uint4* A = nullptr;      // forward g^(t << sh); inverse N^-1 g^-(t << sh)
    const uint4* B = nullptr;      // forward g^c; inverse g^-c
    ~CosetTables() { sync_and_free(device, mem); }
};

struct Domain {
    int order_log = 32;  // 2^order_log: order of the initialised root (size bound)
    std::shared_ptr<DomainTables> tables;
    std::vector<std::shared_ptr<CosetTables>> cosets;  // most recently used first, <= MAX_COSETS
};

static constexpr int MAX_DOMAIN_DEVICES = 64;
static std::mutex g_domain_mu;
// never destroyed: freeing device memory during runtime teardown at exit is unsafe
static Domain* g_domains[MAX_DOMAIN_DEVICES];

// the current device's domain (created on first use); caller holds g_domain_mu
static Domain* current_domain(int* dev_out = nullptr) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DOMAIN_DEVICES) return nullptr;
    if (!g_domains[dev]) g_domains[dev] = new Domain();
    if (dev_out) *dev_out = dev;
    return g_domains[dev];
}

__device__ __forceinline__ uint32_t bitrev(uint32_t x, int bits) {
    return bits == 0 ? 0u : (__builtin_bitreverse32(x) >> (32 - bits));
}

// per-stage tables: entry g (stage s = floor(log2(g+1)) + 1, i = g + 1 - 2^(s-1)) holds
// w_(2^L)^(i * 2^(L-s)) = w_(2^s)^i, one exponentiation per entry (init only), times 2^5 (the
// Montgomery form R = 2^256 -> R' = 2^261 of mbls_fr29.hpp), canonical, in the three limb planes
template <class Q, class W>
struct TwPlanesOf {
    Q* a;  // limbs 0-3
    Q* b;  // limbs 4-7
    W* c;  // limb 8
};
using TwPlanes = TwPlanesOf<const uint4, const uint32_t>;  // what the passes read; k_twiddles writes <uint4, uint32_t>
template <class Q = const uint4, class W = const uint32_t, class B>
MBLS_DEV TwPlanesOf<Q, W> tw_planes(B* base, uint32_t count) {
    Q* a = reinterpret_cast<Q*>(base);
    return {a, a + count, reinterpret_cast<W*>(a + 2 * (size_t)count)};
}
static constexpr size_t TW_ENTRY_BYTES = 36;
// 2^5 R mod r (Montgomery form of 32): x * C32 = x 2^5 (R-form products)
static constexpr uint32_t TW_C32[8] = {0xffffffbau, 0x00000045u, 0x0072d846u, 0x1a25272eu,
                                       0x5dbeee8bu, 0xfe2eedcdu, 0x9eefbe41u, 0x4d043f42u};

// b^e by square and multiply (table builds and the coset scaling: one ladder per entry)
MBLS_DEV Fr fr_pow(Fr b, uint64_t e) {
    Fr acc = Fr::one();
    while (e) {
        if (e & 1) acc = acc * b;
        b = sqr(b);
        e >>= 1;
    }
    return acc;
}

__global__ void k_twiddles(uint8_t* table, Fr w, int L, uint32_t count) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    const int s = 32 - __builtin_clz(g + 1);  // floor(log2(g+1)) + 1
    const uint32_t i = g + 1 - (1u << (s - 1));
    Fr c32;
#pragma unroll
    for (int k = 0; k < 8; ++k) c32.v[k] = TW_C32[k];
    const r29::F29 t = r29::unpack(fr_pow(w, (uint64_t)i << (L - s)) * c32);  // w R' mod r, canonical
    const auto P = tw_planes<uint4, uint32_t>(table, count);
    P.a[g] = make_uint4(t.l[0], t.l[1], t.l[2], t.l[3]);
    P.b[g] = make_uint4(t.l[4], t.l[5], t.l[6], t.l[7]);
    P.c[g] = t.l[8];
}

// Lazy butterflies: between the first load and the last store of a transform, values live in
// [0, 2r) (2r < 2^256).  b*w with b < 2r and a canonical twiddle w < r is < r*R, so the
// Montgomery product needs no final subtraction (fips::mul<C, false>); a + t and a - t are
// brought back into [0, 2r) with one conditional 2r correction each (same cost as the
// canonical add / sub).  The last pass stores canonical values.
static constexpr uint32_t NTT_TWO_R[8] = {0x00000002u, 0xfffffffeu, 0xfffcb7fdu, 0xa77b4805u,
                                          0x1343b00au, 0x6673b010u, 0x533afa90u, 0xe7db4ea6u};  // literals
MBLS_DEV Fr add_2r(const Fr& a, const Fr& b) {
    Fr s, d;
    unsigned c = 0, br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s.v[i] = __builtin_addc(a.v[i], b.v[i], c, &c);
#pragma unroll
    for (int i = 0; i < 8; ++i) d.v[i] = __builtin_subc(s.v[i], NTT_TWO_R[i], br, &br);
    const bool keep = !c && br;  // a + b < 2r
#pragma unroll
    for (int i = 0; i < 8; ++i) s.v[i] = keep ? s.v[i] : d.v[i];
    return s;
}
MBLS_DEV Fr sub_2r(const Fr& a, const Fr& b) {
    Fr d;
    unsigned br = 0, c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d.v[i] = __builtin_subc(a.v[i], b.v[i], br, &br);
    const uint32_t mask = 0u - br;  // a < b: add 2r (mod 2^256)
#pragma unroll
    for (int i = 0; i < 8; ++i) d.v[i] = __builtin_addc(d.v[i], NTT_TWO_R[i] & mask, c, &c);
    return d;
}

// an Fr element as two 16-byte words (LDS tile, global data, twiddle tables): element e at
// [2e], [2e + 1] -- 32-bit element indices (transforms <= 2^30, ntt_call) and b128 accesses
MBLS_DEV Fr ld2(const uint4* p, uint32_t e) {
    const uint4 a = p[2 * e], b = p[2 * e + 1];
    return Fr{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
MBLS_DEV void st2(uint4* p, uint32_t e, const Fr& v) {
    p[2 * e] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
    p[2 * e + 1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}
// twiddle entry g of the limb planes
MBLS_DEV r29::F29 ldtw(const TwPlanes& P, uint32_t g) {
    const uint4 x = P.a[g], y = P.b[g];
    return r29::F29{{x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w, P.c[g]}};
}

// Where a pass's tile lies.  A first pass views the polynomial as 2^L rows x 2^colbits columns and
// takes C adjacent columns from lo0: element (row t, column c) at (t << colbits) + lo0 + c, written
// back as contiguous DIT blocks.  A later pass works in place on 2^L rows 2^s0 apart: element (t, c)
// at hi_base + (t << s0) + lo0 + c.
struct Tile {
    uint32_t poly;  // batch member
    uint32_t lo0, hi_base;
};
template <bool FIRST>
MBLS_DEV Tile tile_of(uint32_t id, int log_n, int s0, int L, int logC) {
    const uint32_t tiles_per_poly = (uint32_t)(((size_t)1 << log_n) >> (L + logC));
    const uint32_t lo_tiles = FIRST ? 1u : (1u << s0) >> logC;
    const uint32_t poly = id / tiles_per_poly, tile = id % tiles_per_poly;
    return Tile{poly, (FIRST ? tile : tile % lo_tiles) << logC, FIRST ? 0u : (tile / lo_tiles) << (s0 + L)};
}
// ... and where its finished value (row, c) goes
template <bool FIRST>
MBLS_DEV uint32_t tile_dst(const Tile& g, uint32_t row, uint32_t c, int log_n, int s0, int L) {
    return FIRST ? (bitrev(g.lo0 + c, log_n - L) << L) + row : g.hi_base + (row << s0) + g.lo0 + c;
}

// The stage engine both pass kernels run: stages l0..L of a pass (global stages s0 + l0 .. s0 + L)
// over a tile of 2^L rows x 2^logC columns that lies in LDS as [row][col], rows in DIT order, and
// behind a barrier.  Pairs of stages run as radix-4 (2 x 2) butterflies in registers (one LDS round
// trip and one barrier per pair), an odd last stage as radix-2.  The last stage group hands every
// finished value, still in [0, 2r), to put(row, col, v) straight from registers: no LDS round
// trip, barrier or separate store loop; with no stage to run (l0 > L) the tile itself is handed over.
//
// TRIV is how the first pair of a first pass (l = 1: j = 0, every twiddle but one is 1) skips its
// three products.  Each kernel keeps its own treatment of that pair, behind this one parameter,
// because both sit within a few registers of the limit of 5 waves per SIMD and the register
// allocation follows the form of the source (profiles/ntt_engine/kernels_cmp.txt):
//   from_l  one loop body that decides from l at run time: k_ntt_pass.  Peeled, its first passes
//           grow by a third (2288 -> 3003 instructions for <true, false, false>).
//   peeled  the pair at l = 1 gets a body of its own (always), the others one without the test
//           (never): k_dom_pass.  Deciding at run time, its first passes spill (0 -> 4 registers for
//           <true, false, *>, 1 -> 26 for <true, true, true>).
// Which of the two would be faster for the plain first pass is a question of its own.
enum class TrivPair { from_l, peeled };  // what a kernel asks of tile_stages
enum class Triv { from_l, always, never };  // what tile_stages asks of one stage pair

// stages l, l + 1 of the tile; fin: no stage follows, the outputs go to put
template <bool FIRST, Triv TRIV, class Put>
MBLS_DEV void stage_pair(uint4* lds, const TwPlanes& tw, int l, int s0, int L, int logC, uint32_t lo_base,
                         const Put& put) {
    const uint32_t C = 1u << logC, T = C << L;
    const bool fin = l + 2 > L;
    const uint32_t h = 1u << (l - 1);  // stage l pairs rows (t, t + h), stage l + 1 rows (t, t + 2h)
    const int s = s0 + l;              // global stage of the first of the pair
    const uint32_t t1 = (1u << (s - 1)) - 1, t2 = (1u << s) - 1;  // stage tables s, s + 1
    const uint32_t stride = h * C;
    for (uint32_t u = threadIdx.x; u < T / 4; u += NTT_THREADS) {
        const uint32_t c = u & (C - 1);
        const uint32_t r = u >> logC;
        const uint32_t j = r & (h - 1);
        const uint32_t q = ((r >> (l - 1)) << (l + 1)) + j;
        const uint32_t e0 = q * C + c;
        const uint32_t lo = FIRST ? 0u : lo_base + c;
        const bool triv = TRIV == Triv::from_l ? FIRST && l == 1 : TRIV == Triv::always;
        // twiddles first: their loads do not depend on the tile
        r29::F29 w1, w2, w3;
        const uint32_t jl = (j << s0) + lo;
        if (!triv) {
            w1 = ldtw(tw, t1 + jl);
            w2 = ldtw(tw, t2 + jl);
        }
        w3 = ldtw(tw, t2 + jl + (h << s0));
        Fr x0 = ld2(lds, e0), x1 = ld2(lds, e0 + stride), x2 = ld2(lds, e0 + 2 * stride),
           x3 = ld2(lds, e0 + 3 * stride);
        // stage l: (x0, x1), (x2, x3) share twiddle w_(2^s)^j
        if (!triv) {
            x1 = r29::mul_words(x1, w1);
            x3 = r29::mul_words(x3, w1);
        }
        Fr y0 = add_2r(x0, x1), y1 = sub_2r(x0, x1), y2 = add_2r(x2, x3), y3 = sub_2r(x2, x3);
        // stage l + 1: (y0, y2) with w_(2^(s+1))^j, (y1, y3) with w_(2^(s+1))^(j + h)
        if (!triv) y2 = r29::mul_words(y2, w2);
        y3 = r29::mul_words(y3, w3);
        if (fin) {
            put(q, c, add_2r(y0, y2));
            put(q + 2 * h, c, sub_2r(y0, y2));
            put(q + h, c, add_2r(y1, y3));
            put(q + 3 * h, c, sub_2r(y1, y3));
        } else {
            st2(lds, e0, add_2r(y0, y2));
            st2(lds, e0 + 2 * stride, sub_2r(y0, y2));
            st2(lds, e0 + stride, add_2r(y1, y3));
            st2(lds, e0 + 3 * stride, sub_2r(y1, y3));
        }
    }
}

template <bool FIRST, TrivPair TRIV, class Put>
MBLS_DEV void tile_stages(uint4* lds, const uint8_t* tw_, uint32_t tw_count, int l0, int s0, int L, int logC,
                          uint32_t lo0, const Put& put) {
    const TwPlanes tw = tw_planes(tw_, tw_count);
    const uint32_t C = 1u << logC, T = C << L;
    const uint32_t lo_base = FIRST ? 0u : lo0;
    int l = l0;
    for (; l + 1 <= L; l += 2) {
        if constexpr (TRIV == TrivPair::from_l) stage_pair<FIRST, Triv::from_l>(lds, tw, l, s0, L, logC, lo_base, put);
        else if (FIRST && l == 1) stage_pair<FIRST, Triv::always>(lds, tw, l, s0, L, logC, lo_base, put);
        else stage_pair<FIRST, Triv::never>(lds, tw, l, s0, L, logC, lo_base, put);
        if (l + 2 > L) return;
        __syncthreads();
    }
    if (l == L) {  // one radix-2 stage left
        const uint32_t half = 1u << (l - 1);
        const int s = s0 + l;                     // global stage, m = 2^s
        const uint32_t ts = (1u << (s - 1)) - 1;  // stage table s
        for (uint32_t u = threadIdx.x; u < T / 2; u += NTT_THREADS) {
            const uint32_t c = u & (C - 1);
            const uint32_t r = u >> logC;
            const uint32_t gg = r >> (l - 1);
            const uint32_t j = r & (half - 1);
            const uint32_t t0 = (gg << l) + j, t1 = t0 + half;
            r29::F29 w;  // a lone first stage of a first pass has twiddle 1
            if (l > 1 || !FIRST) w = ldtw(tw, ts + (j << s0) + (FIRST ? 0u : lo_base + c));
            const Fr a = ld2(lds, t0 * C + c);
            Fr b = ld2(lds, t1 * C + c);
            if (l > 1 || !FIRST) b = r29::mul_words(b, w);
            put(t0, c, add_2r(a, b));
            put(t1, c, sub_2r(a, b));
        }
        return;
    }
    // ---- no stage to run (L == 0, or a first pass whose stages were all replication)
    for (uint32_t e = threadIdx.x; e < T; e += NTT_THREADS) {
        if (FIRST) {
            // block by block: consecutive threads -> consecutive positions of one output block
            const uint32_t p = e & ((1u << L) - 1), c = e >> L;
            put(p, c, ld2(lds, p * C + c));
        } else {
            const uint32_t c = e & (C - 1), t = e >> logC;
            put(t, c, ld2(lds, e));
        }
    }
}

// One pass of up to NTT_TILE_LOG DIT stages of the plain transform: the load phase and the store
// (put) here, the stages in tile_stages.
//   FIRST: stages 1..L with the bit-reversal gather from `in`; else stages s0+1..s0+L in place.
//   LAST:  store canonical values; SCALE (inverse, implies LAST): multiply them by n^-1.
// One tile per workgroup, grid = tiles.  Persistent workgroups walking several tiles lost in every
// form measured in round 6 (profiles/r06/README.md): reload after the stores (11% slower: vmcnt
// counts loads and stores in one in-order counter, so the next tile's first wait also waits for
// this tile's stores), the next tile prefetched into 32 VGPRs during the stage pairs (spills at 4
// workgroups per CU, occupancy at 3: +6-11%), and the next tile LDS-DMA'd behind this tile's
// stores (+7-13%), although a no-store pricing variant shows the stores at ~13% of the pass.
// Index arithmetic is 32-bit (element indices inside a polynomial and the twiddle tables stay
// below 2^31 for transforms <= 2^30), the tile is a uint4 LDS array (every access one b128),
// and the 2r constants are literals (the pass is VALU-issue bound, profiles/r05/ntt_diag.txt).
template <bool FIRST, bool LAST, bool SCALE>
__global__ __launch_bounds__(NTT_THREADS, 5) void k_ntt_pass(uint8_t* __restrict__ out_,
                                                                         const uint8_t* __restrict__ in_,
                                                                         const uint8_t* __restrict__ tw_,
                                                                         uint32_t tw_count, int log_n, int s0, int L,
                                                                         int logC, Fr scale, uint32_t ntiles) {
    __shared__ uint4 lds[NTT_TILE * 2];
    const uint32_t C = 1u << logC;
    const uint32_t T = C << L;  // active tile elements (== NTT_TILE except for tiny transforms)
    const uint32_t colbits = (uint32_t)(log_n - L);
    const uint32_t id = blockIdx.x;  // one tile per workgroup
    if (id >= ntiles) return;
    const Tile g = tile_of<FIRST>(id, log_n, s0, L, logC);
    const size_t poly = (size_t)g.poly << log_n;  // element offset of the tile's polynomial
    const uint4* in = reinterpret_cast<const uint4*>(FIRST ? in_ : out_);
    uint4* o = reinterpret_cast<uint4*>(out_) + 2 * poly;
    // ---- the tile into LDS as [row t][col c] (FIRST: rows at their bit-reversed DIT position; not
    // vectorised: the loop vectoriser split the b128 LDS stores into b32)
#pragma clang loop vectorize(disable) interleave(disable)
    for (uint32_t e = threadIdx.x; e < T; e += NTT_THREADS) {
        const uint32_t c = e & (C - 1), t = e >> logC;
        st2(lds, FIRST ? bitrev(t, L) * C + c : e,
            ld2(in + 2 * poly, FIRST ? (t << colbits) + g.lo0 + c : g.hi_base + (t << s0) + g.lo0 + c));
    }
    __syncthreads();
    auto put = [&](uint32_t row, uint32_t c, Fr v) {
        if (SCALE) v = v * scale;  // v < 2r, scale < r: the reduced product is canonical
        else if (LAST) reduce_once(v);
        st2(o, tile_dst<FIRST>(g, row, c, log_n, s0, L), v);
    };
    tile_stages<FIRST, TrivPair::from_l>(lds, tw_, tw_count, 1, s0, L, logC, g.lo0, put);
}

__global__ void k_copy_scale(uint8_t* out, const uint8_t* in, size_t count, Fr scale, int do_scale) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= count) return;
    Fr v = load<FrCfg>(in + 32 * i);
    if (do_scale) v = v * scale;
    store<FrCfg>(out + 32 * i, v);
}

// ---- host-side field helpers (tiny, init-time only) ----------------------------------
typedef unsigned __int128 u128;
static const uint64_t HFR_P[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL,
                                  0x73eda753299d7d48ULL};
static const uint64_t HFR_ONE[4] = {0x00000001fffffffeULL, 0x5884b7fa00034802ULL, 0x998c4fefecbc4ff5ULL,
                                    0x1824b159acc5056fULL};
static const uint64_t HFR_R2[4] = {0xc999e990f3f29c6dULL, 0x2b6cedcb87925c23ULL, 0x05d314967254398fULL,
                                   0x0748d9d99f59ff11ULL};

static void hfr_mul(uint64_t* r, const uint64_t* a, const uint64_t* b) {
    uint64_t t[6] = {0};
    for (int i = 0; i < 4; ++i) {
        uint64_t c = 0;
        for (int j = 0; j < 4; ++j) {
            u128 s = (u128)a[j] * b[i] + t[j] + c;
            t[j] = (uint64_t)s;
            c = (uint64_t)(s >> 64);
        }
        u128 s = (u128)t[4] + c;
        t[4] = (uint64_t)s;
        t[5] = (uint64_t)(s >> 64);
        uint64_t q = t[0] * 0xfffffffeffffffffULL;
        s = (u128)q * HFR_P[0] + t[0];
        c = (uint64_t)(s >> 64);
        for (int j = 1; j < 4; ++j) {
            s = (u128)q * HFR_P[j] + t[j] + c;
            t[j - 1] = (uint64_t)s;
            c = (uint64_t)(s >> 64);
        }
        s = (u128)t[4] + c;
        t[3] = (uint64_t)s;
        t[4] = t[5] + (uint64_t)(s >> 64);
    }
    bool ge = t[4] != 0;
    if (!ge) {
        ge = true;
        for (int i = 3; i >= 0; --i)
            if (t[i] != HFR_P[i]) {
                ge = t[i] > HFR_P[i];
                break;
            }
    }
    if (ge) {
        uint64_t br = 0;
        for (int i = 0; i < 4; ++i) {
            u128 d = (u128)t[i] - HFR_P[i] - br;
            t[i] = (uint64_t)d;
            br = (uint64_t)(d >> 64) & 1;
        }
    }
    memcpy(r, t, 32);
}

static bool hfr_eq(const uint64_t* a, const uint64_t* b) { return memcmp(a, b, 32) == 0; }

static void hfr_pow(uint64_t* r, const uint64_t* a, const uint64_t* e) {
    uint64_t acc[4];
    memcpy(acc, HFR_ONE, 32);
    for (int i = 255; i >= 0; --i) {
        hfr_mul(acc, acc, acc);
        if ((e[i / 64] >> (i % 64)) & 1) hfr_mul(acc, acc, a);
    }
    memcpy(r, acc, 32);
}

static void hfr_inv(uint64_t* r, const uint64_t* a) {
    uint64_t e[4];
    memcpy(e, HFR_P, 32);
    e[0] -= 2;
    hfr_pow(r, a, e);
}

// order of `w` (Montgomery) as a power of two, or -1
static int hfr_log_order(const uint64_t* w) {
    uint64_t x[4];
    memcpy(x, w, 32);
    for (int k = 0; k <= 32; ++k) {
        if (hfr_eq(x, HFR_ONE)) return k;
        hfr_mul(x, x, x);
    }
    return -1;
}

static void canonical_omega(uint64_t* w, int log_n) {
    memcpy(w, ROOT_2_32_MONT, 32);
    for (int k = log_n; k < 32; ++k) hfr_mul(w, w, w);
}

static Fr to_dev(const uint64_t* h) {
    Fr r;
    memcpy(r.v, h, 32);
    return r;
}

// (re)build the stage tables of `dom` (the current device's) up to 2^max_log; caller holds
// g_domain_mu.  A superseded table stays alive while any snapshot of it does (DomainTables);
// the domain's own reference moves to *old, which the caller drops AFTER releasing the lock
// (the destructor's device synchronisation must not run under g_domain_mu: ADVICE r4)
static eIcicleError build_domain(Domain& dom, int max_log, hipStream_t st, std::shared_ptr<DomainTables>& old) {
    if (dom.tables && dom.tables->max_log >= max_log) return MBLS_SUCCESS;
    const int order = dom.order_log;
    if (max_log > order) return MBLS_INVALID_ARGUMENT;
    size_t count = ((size_t)1 << max_log) - 1;
    if (count == 0) count = 1;
    auto t = std::make_shared<DomainTables>();
    MBLS_TRY(hipGetDevice(&t->device));
    MBLS_TRY(hipMalloc(&t->tw, TW_ENTRY_BYTES * count));
    MBLS_TRY(hipMalloc(&t->tw_inv, TW_ENTRY_BYTES * count));
    t->count = (uint32_t)count;
    uint64_t w[4], wi[4];
    canonical_omega(w, max_log);
    hfr_inv(wi, w);
    int blocks = (int)((count + 255) / 256);
    hipLaunchKernelGGL(k_twiddles, dim3(blocks), dim3(256), 0, st, t->tw, to_dev(w), max_log, (uint32_t)count);
    hipLaunchKernelGGL(k_twiddles, dim3(blocks), dim3(256), 0, st, t->tw_inv, to_dev(wi), max_log, (uint32_t)count);
    MBLS_TRY(hipGetLastError());
    MBLS_TRY(hipStreamSynchronize(st));
    t->max_log = max_log;
    old = std::move(dom.tables);
    dom.tables = std::move(t);
    return MBLS_SUCCESS;
}

// The domain as one call sees it: under the lock, bound the size by the initialised root's order,
// build or extend this device's stage tables when they are too short (init_domain builds up to
// 2^22), and snapshot them; the snapshot stays valid for the whole enqueue.  `superseded` takes an
// extension's old tables: the caller lets it go outside the lock (build_domain).
struct CosetWant {  // the coset tables a domain transform takes under the same lock (coset_tables)
    const uint64_t* g;
    int sh;
    bool inverse;
    std::shared_ptr<CosetTables> got, evicted;  // evicted: let go outside the lock, as superseded
};
static eIcicleError coset_tables(Domain& dom, int log_n, hipStream_t st, CosetWant& w);
static eIcicleError domain_snapshot(int log_n, hipStream_t st, std::shared_ptr<DomainTables>& tables,
                                    std::shared_ptr<DomainTables>& superseded, CosetWant* coset = nullptr) {
    std::lock_guard<std::mutex> lk(g_domain_mu);
    Domain* dom = current_domain();
    if (!dom) return MBLS_INVALID_DEVICE;
    if (log_n > dom->order_log) return MBLS_INVALID_ARGUMENT;  // beyond the initialised root
    if (!dom->tables || dom->tables->max_log < log_n) {
        int want = log_n < 20 ? 20 : log_n;
        if (want > dom->order_log) want = dom->order_log;
        eIcicleError er = build_domain(*dom, want, st, superseded);
        if (er != MBLS_SUCCESS) return er;
    }
    tables = dom->tables;
    return coset ? coset_tables(*dom, log_n, st, *coset) : MBLS_SUCCESS;
}

// n^-1 for n = 2^log_n, Montgomery form
static void hfr_ninv(uint64_t* r, int log_n) {
    uint64_t nm[4] = {(uint64_t)1 << log_n, 0, 0, 0};
    hfr_mul(nm, nm, HFR_R2);  // n in Montgomery form
    hfr_inv(r, nm);
}

// A caller's coset generator into g: 1 a coset, 0 none (no generator, or 1), -1 not a generator --
// zero mod r (a zero-initialised NTTConfig) has no inverse and spans no coset
static int coset_kind(const mbls_fr_t* coset_gen, uint64_t* g) {
    if (!coset_gen) return 0;
    memcpy(g, coset_gen->limbs, 32);
    uint64_t gr[4];
    hfr_mul(gr, g, HFR_R2);  // g R mod r, canonical for any 256-bit g
    const uint64_t zero[4] = {0, 0, 0, 0};
    if (hfr_eq(gr, zero)) return -1;
    return hfr_eq(g, HFR_ONE) ? 0 : 1;
}

static constexpr int NTT_MAX_LOG = 30;    // sizes are ints, element indices 32-bit
static constexpr int NTT_MAX_PASSES = 4;  // ceil(30 / 8)

// a pass's grid: tiles per polynomial times batch members (below 2^31 for every pass pass_plan returns)
static size_t pass_tiles(int log_n, int L, int logC, int batch) {
    return (((size_t)1 << log_n) >> (L + logC)) * (size_t)batch;
}

// The pass plan of a transform of 2^log_n, (s0, L, logC) per pass: the log_n stages split into
// ceil(log_n / NTT_PASS_STAGES) passes of near-equal stage counts L (tile rows 2^L), each tile with
// as many adjacent columns 2^logC as the tile size and the available column count allow (8 stages
// leave >= 4 columns: >= 128-byte contiguous row segments in HBM).  Returns the pass count (0 for
// log_n == 0), or -1 where a pass's tile count times `batch`, its grid, would reach 2^31.
static int pass_plan(int log_n, int batch, int (*pl)[3]) {
    const int npass = (log_n + NTT_PASS_STAGES - 1) / NTT_PASS_STAGES;
    int s0 = 0;
    for (int p = 0; p < npass; ++p) {
        const int remaining = log_n - s0;
        const int L = (remaining + (npass - p) - 1) / (npass - p);
        const int colspace = p == 0 ? (log_n - L) : s0;
        int logC = NTT_TILE_LOG - L;
        if (logC > colspace) logC = colspace;
        if (pass_tiles(log_n, L, logC, batch) > 0x7fffffff) return -1;
        pl[p][0] = s0, pl[p][1] = L, pl[p][2] = logC;
        s0 += L;
    }
    return npass;
}

// one k_ntt_pass over `batch` polynomials of 2^log_n in `out` (a first pass gathers from `in`)
static eIcicleError launch_ntt_pass(bool first, bool last, bool inverse, uint8_t* out, const uint8_t* in,
                                    const uint8_t* tw, uint32_t tw_count, int log_n, const int* pl, Fr scale, int batch,
                                    hipStream_t st) {
    const int s0 = pl[0], L = pl[1], logC = pl[2];
    const uint32_t nt = (uint32_t)pass_tiles(log_n, L, logC, batch);
    auto* k = k_ntt_pass<false, false, false>;
    if (first && last) k = inverse ? k_ntt_pass<true, true, true> : k_ntt_pass<true, true, false>;
    else if (first) k = k_ntt_pass<true, false, false>;
    else if (last) k = inverse ? k_ntt_pass<false, true, true> : k_ntt_pass<false, true, false>;
    hipLaunchKernelGGL(k, dim3(nt), dim3(NTT_THREADS), 0, st, out, in, tw, tw_count, log_n, s0, L, logC, scale, nt);
    MBLS_TRY(hipGetLastError());
    return MBLS_SUCCESS;
}

// enqueue forward/inverse NTT of `batch` polynomials of 2^log_n on device buffers
// (D: the caller's snapshot of the domain tables, kept alive across the enqueue)
eIcicleError ntt_device(uint8_t* out, const uint8_t* in, int log_n, bool inverse, int batch, const DomainTables& D,
                        hipStream_t st) {
    if (!D.tw || log_n > D.max_log || log_n > NTT_MAX_LOG) return MBLS_INVALID_ARGUMENT;
    int pl[NTT_MAX_PASSES][3];
    const int np = pass_plan(log_n, batch, pl);
    if (np < 0) return MBLS_INVALID_ARGUMENT;
    uint64_t ninv_h[4];
    memcpy(ninv_h, HFR_ONE, 32);
    if (inverse) hfr_ninv(ninv_h, log_n);
    const Fr scale = to_dev(ninv_h);
    if (np == 0) {
        size_t cnt = (size_t)batch;
        hipLaunchKernelGGL(k_copy_scale, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, out, in, cnt, scale, 0);
        MBLS_TRY(hipGetLastError());
        return MBLS_SUCCESS;
    }
    ProfScope prof_t("ntt.transform", st);
    for (int p = 0; p < np; ++p) {
        ProfScope prof_p("ntt.pass", st);
        const eIcicleError er = launch_ntt_pass(p == 0, p == np - 1, inverse, out, in, inverse ? D.tw_inv : D.tw, D.count,
                                                log_n, pl[p], scale, batch, st);
        if (er != MBLS_SUCCESS) return er;
    }
    return MBLS_SUCCESS;
}

static int log2_exact(long long n) {
    if (n <= 0 || (n & (n - 1))) return -1;
    int k = 0;
    while ((1LL << k) < n) ++k;
    return k;
}

eIcicleError ntt_init_domain(const mbls_fr_t* root, const NTTInitDomainConfig* cfg) {
    if (!root) return MBLS_INVALID_POINTER;
    hipStream_t st = cfg ? static_cast<hipStream_t>(cfg->stream) : nullptr;
    // The root only sizes the domain: its order 2^K (read as Montgomery, else as standard
    // form).  Twiddles are always the canonical best_fft roots (see file header).
    int K = hfr_log_order(root->limbs);
    if (K < 0) {
        uint64_t m[4];
        hfr_mul(m, root->limbs, HFR_R2);
        K = hfr_log_order(m);
    }
    if (K < 0) return MBLS_INVALID_ARGUMENT;
    std::shared_ptr<DomainTables> old;  // dropped after the lock (declared before it)
    std::lock_guard<std::mutex> lk(g_domain_mu);
    Domain* dom = current_domain();
    if (!dom) return MBLS_INVALID_DEVICE;
    // the tables are canonical (independent of the root): a smaller order only bounds sizes
    dom->order_log = K;
    // stage tables up to 2^22 now (2 x 128 MiB); larger sizes extend them on first use
    return build_domain(*dom, K < 22 ? K : 22, st, old);
}

eIcicleError ntt_release_domain() {
    std::shared_ptr<DomainTables> old;
    std::vector<std::shared_ptr<CosetTables>> old_cosets;
    {
        std::lock_guard<std::mutex> lk(g_domain_mu);
        Domain* dom = current_domain();
        if (!dom) return MBLS_INVALID_DEVICE;
        old_cosets.swap(dom->cosets);
        old = std::move(dom->tables);
        dom->tables.reset();
        dom->order_log = 32;
    }
    return MBLS_SUCCESS;  // `old` frees the tables here unless a transform still holds them
}

// coset scaling x_i *= g^(+-i) within each polynomial (device, in place)
__global__ void k_coset_scale(uint8_t* data, Fr g, size_t n, size_t total) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    Fr v = load<FrCfg>(data + 32 * i);
    store<FrCfg>(data + 32 * i, v * fr_pow(g, i & (n - 1)));
}

// Layout permutation (gather): out position q of layout (out_cols, out_rev) takes the element
// of layout (in_cols, in_rev) holding the same (member b, natural index e).  *_cols: column-
// major batch (element e of member b at e*batch + b); *_rev: bit-reversed element order.
__global__ void k_perm(uint8_t* __restrict__ out, const uint8_t* __restrict__ in, int log_n, uint32_t batch,
                       int out_cols, int out_rev, int in_cols, int in_rev) {
    const size_t n = (size_t)1 << log_n;
    const size_t total = n * batch;
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
        const size_t b = out_cols ? q % batch : q >> log_n;
        const size_t i = out_cols ? q / batch : q & (n - 1);
        const size_t e = out_rev ? bitrev((uint32_t)i, log_n) : i;
        const size_t pi = in_rev ? bitrev((uint32_t)e, log_n) : e;
        const size_t src = in_cols ? pi * batch + b : (b << log_n) + pi;
        store<FrCfg>(out + 32 * q, load<FrCfg>(in + 32 * src));
    }
}

static eIcicleError launch_perm(uint8_t* out, const uint8_t* in, int log_n, int batch, bool out_cols, bool out_rev,
                                bool in_cols, bool in_rev, hipStream_t st) {
    const size_t total = ((size_t)1 << log_n) * (size_t)batch;
    size_t blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(k_perm, dim3((unsigned)blocks), dim3(256), 0, st, out, in, log_n, (uint32_t)batch,
                       out_cols ? 1 : 0, out_rev ? 1 : 0, in_cols ? 1 : 0, in_rev ? 1 : 0);
    MBLS_TRY(hipGetLastError());
    return MBLS_SUCCESS;
}

// Full ICICLE-semantics NTT call: staging, batch (row or columns_batch layout), coset,
// orderings.  R = bit-reversed order; M ("mixed", implementation-defined in ICICLE) is
// bit-reversed here too, so kNM -> kMN round-trips.  Non-natural layouts are permuted to
// natural row-major around the natural-order transform (one extra HBM pass each).
eIcicleError ntt_call(const mbls_fr_t* input, int size, NTTDir dir, const NTTConfig* cfg, mbls_fr_t* output,
                      const mbls_fr_t* coset_gen) {
    if (!input || !output || !cfg) return MBLS_INVALID_POINTER;
    int log_n = log2_exact(size);
    if (log_n < 0) return MBLS_INVALID_ARGUMENT;
    const int ord = (int)cfg->ordering;
    if (ord < MBLS_ORDERING_NN || ord > MBLS_ORDERING_MN) return MBLS_INVALID_ARGUMENT;
    // coset: forward evaluates on g*H (pre-scale by g^i); inverse post-scales by g^-i
    uint64_t g[4];
    const int kind = coset_kind(coset_gen, g);
    if (kind < 0) return MBLS_INVALID_ARGUMENT;
    const bool coset = kind > 0;
    const bool in_rev = ord == MBLS_ORDERING_RN || ord == MBLS_ORDERING_RR || ord == MBLS_ORDERING_MN;
    const bool out_rev = ord == MBLS_ORDERING_NR || ord == MBLS_ORDERING_RR || ord == MBLS_ORDERING_NM;
    const bool cols = cfg->columns_batch;
    int batch = cfg->batch_size > 0 ? cfg->batch_size : 1;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    std::shared_ptr<DomainTables> tables, superseded;
    eIcicleError er = domain_snapshot(log_n, st, tables, superseded);
    if (er != MBLS_SUCCESS) return er;
    const size_t bytes = (size_t)size * 32 * (size_t)batch;
    const size_t total = (size_t)size * batch;
    const bool inverse = (dir == MBLS_NTT_INVERSE);
    const bool perm_in = (in_rev || cols) && log_n > 0;
    const bool perm_out = (out_rev || cols) && log_n > 0;
    const bool in_dev = cfg->are_inputs_on_device, out_dev = cfg->are_outputs_on_device;
    // the transform's source must be natural row-major, writable when coset-scaled, and
    // distinct from its destination (the first pass gathers bit-reversed)
    const bool same = in_dev && out_dev && input == output;
    const bool work_in_tmp = perm_in || (coset && !inverse) || (same && !perm_out);

    // a transform that needs no staging (device in / out, natural order, distinct buffers: the
    // prover's shape) takes no scratch context (Staging::LEASE_IF_STAGED): the lease's `done`
    // event would hold the next dispatch ~5 us, 1% of a 2^22 transform
    Staging S(st, Staging::LEASE_IF_STAGED);
    const uint8_t* src;
    uint8_t *dst, *wout = nullptr, *t = nullptr;
    S.in(&src, input, bytes, in_dev);
    S.out(&dst, output, bytes, out_dev);
    if (perm_out) S.scratch(&wout, bytes);
    if (work_in_tmp) S.scratch(&t, bytes);
    if ((er = S.open()) != MBLS_SUCCESS) return er;
    if (!perm_out) wout = dst;
    const uint8_t* win = src;
    if (work_in_tmp) {
        if (perm_in) {
            if ((er = launch_perm(t, src, log_n, batch, false, false, cols, in_rev, st)) != MBLS_SUCCESS) return er;
        } else {
            MBLS_TRY(hipMemcpyAsync(t, src, bytes, hipMemcpyDeviceToDevice, st));
        }
        if (coset && !inverse) {
            hipLaunchKernelGGL(k_coset_scale, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, t, to_dev(g),
                               (size_t)size, total);
            MBLS_TRY(hipGetLastError());
        }
        win = t;
    }
    er = ntt_device(wout, win, log_n, inverse, batch, *tables, st);
    if (er != MBLS_SUCCESS) return er;
    if (coset && inverse) {
        uint64_t gi[4];
        hfr_inv(gi, g);
        hipLaunchKernelGGL(k_coset_scale, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, wout, to_dev(gi),
                           (size_t)size, total);
        MBLS_TRY(hipGetLastError());
    }
    if (perm_out && (er = launch_perm(dst, wout, log_n, batch, cols, out_rev, false, false, st)) != MBLS_SUCCESS)
        return er;
    // a staged host input is out of the caller's memory once hipMemcpyAsync returns (pageable)
    // or is the caller's to keep alive (pinned): only a host result forces the wait
    return S.close(cfg->is_async);
}

// The EC-NTT's view of the domain (mbls_common.hpp; ecntt.hip): the order bound and the canonical
// roots only -- it neither builds nor extends the stage tables.
eIcicleError ntt_domain_roots(int log_n, bool inverse, uint64_t* w, uint64_t* n_inv) {
    {
        std::lock_guard<std::mutex> lk(g_domain_mu);
        Domain* dom = current_domain();
        if (!dom) return MBLS_INVALID_DEVICE;
        if (log_n > dom->order_log) return MBLS_INVALID_ARGUMENT;  // beyond the initialised root
    }
    canonical_omega(w, log_n);
    if (inverse) hfr_inv(w, w);
    hfr_ninv(n_inv, log_n);
    return MBLS_SUCCESS;
}
bool fr_is_montgomery_one(const uint64_t* a) { return hfr_eq(a, HFR_ONE); }

// ---------------------------------------------------------------------------------------------
// Extended-coset transforms: halo2's EvaluationDomain::coeff_to_extended and extended_to_coeff
// (DESIGN.md 5.12).  The plan (pass_plan), the tiles, the twiddles and the stage engine (tile_stages)
// are the plain transform's.  k_dom_pass adds what the first and the last pass do differently -- its
// own load phase, a first stage past the replicated ones, and its own put -- and the passes between
// them are k_ntt_pass<false, ...> as they stand (launch_ntt_pass).
//
// Forward (size coefficients -> N = 2^K values on g H_N), E = K - log2(next_pow2(size)):
//   the first pass's tile rows are the indices (t << colbits) + col, so only rows t < 2^(L - Ee),
//   Ee = min(E, L), can hold a coefficient.  They are loaded (an index >= size reads as zero),
//   multiplied by g^i, and written to their bit-reversed row p << Ee and to the 2^Ee - 1 rows below
//   it: DIT stages 1..Ee of a group whose other inputs are zero only copy ((a, 0) -> (a, a)).  The
//   butterflies start at stage Ee + 1.  For E > L the pruning is capped at the first pass: the
//   second pass runs in full.  The output buffer is the working buffer: no scratch.
// Inverse (N values -> out_size coefficients): the first pass multiplies by vanishing_inv[j mod
//   period] on load, the last pass multiplies every output by N^-1 g^-i and stores i < out_size.
//   A transform of more than one pass works in an N-element scratch array per member.
// Coset powers: the index splits as the tile does, i = (t << sh) + c (forward sh = colbits of the
//   first pass, inverse sh = s0 of the last), so g^(+-i) = A[t] B[c] with two small tables
//   (2^(K - sh) and 2^sh entries; 2^8 + 2^14 forward and 2^7 + 2^15 inverse at 2^22) and two
//   products per element.  The tables are cached in the device's domain, keyed by (generator, K,
//   sh, direction): a prover uses one generator for the whole proof, and a cached table lets the
//   forward call run without a scratch lease (whose event would hold the next dispatch ~5 us).
// Lazy range: a loaded value is canonical (the input contract) and the table entries are canonical,
//   so each reducing Montgomery product (Fr operator*, a < 2r, b < r -> canonical) enters the tile
//   below r, inside the butterflies' [0, 2r).  The last pass's values are < 2r and its first product
//   is by a canonical A[t]: canonical, as the SCALE product of k_ntt_pass.
struct DomArgs {
    uint32_t in_stride, out_stride;  // elements between batch members
    uint32_t in_size;                // forward FIRST: coefficients per member
    uint32_t out_size;               // inverse LAST: coefficients kept per member
    int E;                           // forward FIRST: replication stages skipped (<= L)
    int sh;                          // coset index split
    const uint4* tabA;               // CosetTables::A, or null: no coset
    const uint4* tabB;               // CosetTables::B
    const uint4* vinv;               // inverse FIRST: vanishing_inv, or null
    uint32_t vmask;                  // period - 1
    Fr scale;                        // inverse LAST without a coset: N^-1
};

template <bool FIRST, bool LAST, bool INV>
__global__ __launch_bounds__(NTT_THREADS, 5) void k_dom_pass(uint8_t* __restrict__ out_,
                                                                         const uint8_t* __restrict__ in_,
                                                                         const uint8_t* __restrict__ tw_,
                                                                         uint32_t tw_count, int log_n, int s0, int L,
                                                                         int logC, uint32_t ntiles, DomArgs A) {
    __shared__ uint4 lds[NTT_TILE * 2];
    const uint32_t C = 1u << logC;
    const uint32_t T = C << L;
    const uint32_t colbits = (uint32_t)(log_n - L);
    const uint32_t id = blockIdx.x;  // one tile per workgroup
    if (id >= ntiles) return;
    const Tile g = tile_of<FIRST>(id, log_n, s0, L, logC);
    const uint4* in = reinterpret_cast<const uint4*>(in_) + 2 * (size_t)g.poly * A.in_stride;
    uint4* o = reinterpret_cast<uint4*>(out_) + 2 * (size_t)g.poly * A.out_stride;
    const uint32_t smask = (1u << A.sh) - 1;
    const int Ee = (FIRST && !INV) ? A.E : 0;

    if (FIRST) {
        // rows t < 2^(L - Ee) only; each lands on its bit-reversed DIT row and its replicas
        const uint32_t Tl = T >> Ee;
#pragma clang loop vectorize(disable) interleave(disable)
        for (uint32_t e = threadIdx.x; e < Tl; e += NTT_THREADS) {
            const uint32_t c = e & (C - 1), t = e >> logC;
            const uint32_t idx = (t << colbits) + g.lo0 + c;
            Fr v;
            if (INV) {
                v = ld2(in, idx);
                if (A.vinv) v = v * ld2(A.vinv, idx & A.vmask);  // canonical * canonical
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) v.v[k] = 0;
                if (idx < A.in_size) v = ld2(in, idx);
                // canonical v times canonical g^(t << sh), then times canonical g^c: canonical
                if (A.tabA) v = (v * ld2(A.tabA, idx >> A.sh)) * ld2(A.tabB, idx & smask);
            }
            const uint32_t p = bitrev(t, L - Ee) << Ee;
            for (uint32_t r = 0; r < (1u << Ee); ++r) st2(lds, (p + r) * C + c, v);
        }
    } else {
#pragma clang loop vectorize(disable) interleave(disable)
        for (uint32_t e = threadIdx.x; e < T; e += NTT_THREADS)
            st2(lds, e, ld2(in, g.hi_base + ((e >> logC) << s0) + g.lo0 + (e & (C - 1))));
    }
    __syncthreads();
    // the last store of a finished value, at position dst of its member
    auto put = [&](uint32_t row, uint32_t c, Fr v) {
        const uint32_t dst = tile_dst<FIRST>(g, row, c, log_n, s0, L);
        if (INV && LAST) {
            // v < 2r: the first product is by a canonical factor and reduces
            if (A.tabA) v = (v * ld2(A.tabA, dst >> A.sh)) * ld2(A.tabB, dst & smask);
            else v = v * A.scale;
            if (dst < A.out_size) st2(o, dst, v);
        } else {
            if (LAST) reduce_once(v);
            st2(o, dst, v);
        }
    };
    // the replicated stages 1..Ee are done: the butterflies start at Ee + 1
    tile_stages<FIRST, TrivPair::peeled>(lds, tw_, tw_count, Ee + 1, s0, L, logC, g.lo0, put);
}

// size-1 transforms: out = in (* vanishing_inv[0]); g^0 = N^-1 = 1
__global__ void k_dom_point(uint8_t* out, const uint8_t* in, const uint8_t* vinv, size_t count) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= count) return;
    Fr v = load<FrCfg>(in + 32 * i);
    if (vinv) v = v * load<FrCfg>(vinv);
    store<FrCfg>(out + 32 * i, v);
}

// A[t] = scale * g^(t << sh), t < nA;  B[c] = g^c, c < nB (one ladder per table entry, build only)
__global__ void k_dom_tables(uint8_t* A, uint32_t nA, uint8_t* B, uint32_t nB, Fr g, int sh, Fr scale) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nA + nB) return;
    const Fr acc = fr_pow(g, i < nA ? (uint64_t)i << sh : (uint64_t)(i - nA));
    if (i < nA) store<FrCfg>(A + 32 * (size_t)i, acc * scale);
    else store<FrCfg>(B + 32 * (size_t)(i - nA), acc);
}

static constexpr size_t MAX_COSETS = 8;

static int ceil_log2(long long n) {
    int k = 0;
    while ((1LL << k) < n) ++k;
    return k;
}

static eIcicleError domain_plan(int size, int extended_size, int32_t* out) {
    if (!out) return MBLS_INVALID_POINTER;
    const int K = log2_exact(extended_size);
    if (K < 0 || K > NTT_MAX_LOG || size < 1 || size > extended_size) return MBLS_INVALID_ARGUMENT;
    int pl[NTT_MAX_PASSES][3];
    const int np = pass_plan(K, 1, pl);
    const int E = K - ceil_log2(size);
    const int L0 = np ? pl[0][1] : 0;
    const int Ee = E < L0 ? E : L0;
    out[0] = np;
    out[1] = E;
    out[2] = Ee;
    out[3] = 1 << (L0 - Ee);
    out[4] = 0;                      // the forward call works in its output
    out[5] = np > 1 ? 1 << K : 0;    // elements of 32 bytes (2^30 of them would not fit as bytes)
    for (int p = 0; p < np; ++p)
        for (int k = 0; k < 3; ++k) out[6 + 3 * p + k] = pl[p][k];
    return MBLS_SUCCESS;
}

// the coset tables of (g, log_n, sh, inverse) on the current device, built on `st` (and waited
// for, once) when the cache lacks them; caller holds g_domain_mu (domain_snapshot).  w.evicted takes a
// table pushed out of the cache: the caller lets it go outside the lock (its destructor synchronises).
static eIcicleError coset_tables(Domain& dom, int log_n, hipStream_t st, CosetWant& w) {
    const uint64_t* g = w.g;
    const int sh = w.sh;
    const bool inverse = w.inverse;
    std::shared_ptr<CosetTables>&got = w.got, &evicted = w.evicted;
    for (size_t k = 0; k < dom.cosets.size(); ++k) {
        const CosetTables& c = *dom.cosets[k];
        if (c.log_n == log_n && c.sh == sh && c.inverse == inverse && hfr_eq(c.g, g)) {
            got = dom.cosets[k];
            dom.cosets.erase(dom.cosets.begin() + k);
            dom.cosets.insert(dom.cosets.begin(), got);
            return MBLS_SUCCESS;
        }
    }
    auto t = std::make_shared<CosetTables>();
    MBLS_TRY(hipGetDevice(&t->device));
    const uint32_t nA = 1u << (log_n - sh), nB = 1u << sh;
    MBLS_TRY(hipMalloc(&t->mem, 32 * ((size_t)nA + nB)));
    memcpy(t->g, g, 32);
    t->log_n = log_n, t->sh = sh, t->inverse = inverse;
    t->A = reinterpret_cast<const uint4*>(t->mem);
    t->B = t->A + 2 * (size_t)nA;
    uint64_t base[4], scale[4];
    memcpy(base, g, 32);
    memcpy(scale, HFR_ONE, 32);
    if (inverse) {
        hfr_inv(base, g);
        hfr_ninv(scale, log_n);
    }
    hipLaunchKernelGGL(k_dom_tables, dim3((nA + nB + 255) / 256), dim3(256), 0, st, t->mem, nA, t->mem + 32 * (size_t)nA,
                       nB, to_dev(base), sh, to_dev(scale));
    MBLS_TRY(hipGetLastError());
    MBLS_TRY(hipStreamSynchronize(st));  // another stream may use the cached tables next
    dom.cosets.insert(dom.cosets.begin(), t);
    if (dom.cosets.size() > MAX_COSETS) {
        evicted = std::move(dom.cosets.back());
        dom.cosets.pop_back();
    }
    got = std::move(t);
    return MBLS_SUCCESS;
}

// Both directions: validation (before any HIP call), the domain's tables, staging, the passes.
//   forward: input = coeffs (in_count = size), output = N values; vinv unused
//   inverse: input = N evaluations, output = out_count coefficients
static eIcicleError domain_call(bool inverse, const mbls_fr_t* input, int in_count, int extended_size, int out_count,
                                const mbls_fr_t* coset_gen, const mbls_fr_t* vanishing_inv, int period,
                                const NTTConfig* cfg, mbls_fr_t* output) {
    if (!input || !output || !cfg) return MBLS_INVALID_POINTER;
    const int K = log2_exact(extended_size);
    if (K < 0 || K > NTT_MAX_LOG) return MBLS_INVALID_ARGUMENT;
    const int part = inverse ? out_count : in_count;  // size or out_size
    if (part < 1 || part > extended_size) return MBLS_INVALID_ARGUMENT;
    if (cfg->columns_batch || (int)cfg->ordering != MBLS_ORDERING_NN) return MBLS_INVALID_ARGUMENT;
    if (inverse && vanishing_inv && (log2_exact(period) < 0 || period > extended_size)) return MBLS_INVALID_ARGUMENT;
    uint64_t g[4];
    const int kind = coset_kind(coset_gen, g);
    if (kind < 0) return MBLS_INVALID_ARGUMENT;
    const int batch = cfg->batch_size > 0 ? cfg->batch_size : 1;
    const size_t N = (size_t)1 << K;
    int pl[NTT_MAX_PASSES][3];
    const int np = pass_plan(K, batch, pl);
    if (np < 0) return MBLS_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(cfg->stream);
    // forward: i = (t << colbits) + c of the first pass; inverse: i = (row << s0) + lo of the last
    const int sh = np ? (inverse ? pl[np - 1][0] : K - pl[0][1]) : 0;

    std::shared_ptr<DomainTables> tables, superseded;
    CosetWant cw{g, sh, inverse, nullptr, nullptr};
    eIcicleError er = domain_snapshot(K, st, tables, superseded, kind > 0 && np ? &cw : nullptr);
    if (er != MBLS_SUCCESS) return er;
    const std::shared_ptr<CosetTables>& ctab = cw.got;
    const bool in_dev = cfg->are_inputs_on_device, out_dev = cfg->are_outputs_on_device;
    const size_t in_stride = inverse ? N : (size_t)in_count, out_stride = inverse ? (size_t)out_count : N;
    Staging S(st, Staging::LEASE_IF_STAGED);
    const uint8_t *src, *vdev = nullptr;
    uint8_t *dst, *work = nullptr;
    S.in(&src, input, in_stride * 32 * batch, in_dev);
    if (inverse && vanishing_inv) S.in(&vdev, vanishing_inv, (size_t)period * 32, in_dev);
    S.out(&dst, output, out_stride * 32 * batch, out_dev);
    if (inverse && np > 1) S.scratch(&work, N * 32 * batch);  // the input is const, the output too short
    if ((er = S.open()) != MBLS_SUCCESS) return er;

    if (np == 0) {
        hipLaunchKernelGGL(k_dom_point, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, dst, src, vdev,
                           (size_t)batch);
        MBLS_TRY(hipGetLastError());
        return S.close(cfg->is_async);
    }
    DomArgs A;
    A.in_stride = (uint32_t)in_stride, A.out_stride = (uint32_t)out_stride;
    A.in_size = (uint32_t)in_count, A.out_size = (uint32_t)out_count;
    const int E = inverse ? 0 : K - ceil_log2(in_count);
    A.E = E < pl[0][1] ? E : pl[0][1];
    A.sh = sh;
    A.tabA = ctab ? ctab->A : nullptr, A.tabB = ctab ? ctab->B : nullptr;
    A.vinv = reinterpret_cast<const uint4*>(vdev), A.vmask = vdev ? (uint32_t)period - 1 : 0;
    uint64_t ninv_h[4];
    memcpy(ninv_h, HFR_ONE, 32);
    if (inverse) hfr_ninv(ninv_h, K);
    A.scale = to_dev(ninv_h);
    const uint8_t* tw = inverse ? tables->tw_inv : tables->tw;
    uint8_t* wbuf = inverse ? work : dst;  // where the passes between the first and the last work
    ProfScope prof_t(inverse ? "domain.extended_to_coeff" : "domain.coeff_to_extended", st);
    for (int p = 0; p < np; ++p) {
        const bool first = p == 0, last = p == np - 1;
        if (!first && !(last && inverse)) {  // the plain transform's pass as it stands
            er = launch_ntt_pass(false, last, inverse, wbuf, wbuf, tw, tables->count, K, pl[p], A.scale, batch, st);
            if (er != MBLS_SUCCESS) return er;
            continue;
        }
        const int s0 = pl[p][0], L = pl[p][1], logC = pl[p][2];
        const uint32_t nt = (uint32_t)pass_tiles(K, L, logC, batch);
        DomArgs a = A;
        if (!first) a.in_stride = (uint32_t)N;
        if (!last) a.out_stride = (uint32_t)N;
        auto* k = k_dom_pass<false, true, true>;
        if (first && last) k = inverse ? k_dom_pass<true, true, true> : k_dom_pass<true, true, false>;
        else if (first) k = inverse ? k_dom_pass<true, false, true> : k_dom_pass<true, false, false>;
        hipLaunchKernelGGL(k, dim3(nt), dim3(NTT_THREADS), 0, st, last ? dst : wbuf, first ? src : wbuf, tw, tables->count,
                           K, s0, L, logC, nt, a);
        MBLS_TRY(hipGetLastError());
    }
    return S.close(cfg->is_async);
}

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError bls12_381_ntt_init_domain_cuda(const mbls_fr_t* root_of_unity, const NTTInitDomainConfig* config) {
    return ntt_init_domain(root_of_unity, config);
}
eIcicleError bls12_381_ntt_release_domain_cuda(void) { return ntt_release_domain(); }
eIcicleError bls12_381_ntt_cuda(const mbls_fr_t* input, int size, NTTDir dir, const NTTConfig* config,
                                mbls_fr_t* output) {
    return ntt_call(input, size, dir, config, output, config ? &config->coset_gen : nullptr);
}
eIcicleError bls12_381_coset_ntt_cuda(const mbls_fr_t* input, int size, NTTDir dir, const mbls_fr_t* coset_gen,
                                      const NTTConfig* config, mbls_fr_t* output) {
    return ntt_call(input, size, dir, config, output, coset_gen);
}
eIcicleError bls12_381_field_ntt_cuda(const mbls_fr_t* input, int size, NTTDir dir, const NTTConfig* config,
                                      mbls_fr_t* output) {
    return ntt_call(input, size, dir, config, output, config ? &config->coset_gen : nullptr);
}
eIcicleError bls12_381_field_ntt_init_domain_cuda(const mbls_fr_t* root_of_unity, const NTTInitDomainConfig* config) {
    return ntt_init_domain(root_of_unity, config);
}
eIcicleError bls12_381_field_ntt_release_domain_cuda(void) { return ntt_release_domain(); }

eIcicleError mbls_fr_coeff_to_extended(const mbls_fr_t* coeffs, int size, int extended_size, const mbls_fr_t* coset_gen,
                                       const NTTConfig* config, mbls_fr_t* output) {
    return domain_call(false, coeffs, size, extended_size, extended_size, coset_gen, nullptr, 0, config, output);
}
eIcicleError mbls_fr_extended_to_coeff(const mbls_fr_t* evals, int extended_size, int out_size,
                                       const mbls_fr_t* coset_gen, const mbls_fr_t* vanishing_inv, int period,
                                       const NTTConfig* config, mbls_fr_t* output) {
    return domain_call(true, evals, extended_size, extended_size, out_size, coset_gen, vanishing_inv, period, config,
                       output);
}
eIcicleError mbls_fr_domain_plan(int size, int extended_size, int32_t* out) {
    return domain_plan(size, extended_size, out);
}

// ICICLE get_root_of_unity_from_domain (registered as NttGetRouFromDomainImpl,
// icicle_backend_api.cuh:135-138): w_(2^logn) of the initialised domain, Montgomery form
eIcicleError bls12_381_ntt_get_rou_from_domain(uint64_t logn, mbls_fr_t* rou) {
    if (!rou) return MBLS_INVALID_POINTER;
    std::lock_guard<std::mutex> lk(g_domain_mu);
    Domain* dom = current_domain();
    if (!dom) return MBLS_INVALID_DEVICE;
    if (!dom->tables || logn > (uint64_t)dom->order_log) return MBLS_INVALID_ARGUMENT;
    canonical_omega(rou->limbs, (int)logn);
    return MBLS_SUCCESS;
}

}  // extern "C"
