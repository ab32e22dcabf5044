// graph.hip -- Fr graph evaluator: one caller-supplied straight-line program of three-address ops
// over named values, run once per row over columns read at rotated rows (mbls_fr_eval_graph).  It
// is the form halo2's GraphEvaluator hands over for custom gates: a list of calculations, each
// writing one intermediate that any later one may read, so a shared subexpression is computed
// once.  The stack form (expr.hip) stays as it is.  No reference counterpart: the reference
// composes these on the CPU.
//
// One launch.  A lane owns one row of a tile of 64 contiguous rows; a workgroup is one wave and
// strides over the tiles.  The host (mbls_graph.hpp) validates the program, finds every value's
// last reader and assigns LDS slots by a linear scan, then resolves the program into 40-byte ops
// in the scratch context: the opcode, where each operand comes from, the row offsets reduced into
// [0, size), and the addresses (column, constant, output member).  Every lane reads the same op, so
// the fetch is uniform and the dispatch is a uniform switch.
//
// Values are never a register array (indexed by the program, it would go to private memory).  The
// result of the previous op is a register value, `prev`; an operand that names it is forwarded from
// there.  A value with a later reader is also written to its slot in LDS, word-major: word w of
// slot s of lane t at ((s * 8 + w) * 64 + t) * 4, so the wave's access to one word is 64 consecutive
// dwords.  A lane only ever touches its own words: no barrier.  Column and constant operands are
// loaded straight into the operation.  A chain in which each value feeds only the next op makes no
// LDS traffic.  The LDS is dynamic, peak slots of 2 KiB: a shallow graph keeps its occupancy.
//
// Columns are witness-derived: no branch and no address depends on a field value.  Rows past the
// end of a partial tile compute on the last row and store nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "mbls_graph.hpp"
#include "mbls_rowprog.hpp"

namespace mbls {

static constexpr int GRAPH_THREADS = 64;                                // one wave: a slot is 2 KiB
static constexpr size_t GRAPH_SLOT_BYTES = 32 * (size_t)GRAPH_THREADS;
static constexpr int GRAPH_MAX_GRID = 256 * 32;  // 32 waves per CU is the residency limit; stride beyond
static_assert(GRAPH_SLOT_BYTES * GRAPH_BUDGET <= 64 * 1024, "the slot file fits one workgroup's LDS");

// a resolved op: what the kernel reads
struct GraphOp {
    uint32_t ctl;    // mbls_fr_graph_opcode | a's GraphFrom << 8 | b's << 12 | result goes to a slot << 16
    uint32_t slots;  // a's slot | b's << 8 | the result's << 16
    uint32_t a_off, b_off;  // COLUMN: (rot * rot_stride) mod size
    const uint8_t *pa, *pb;  // COLUMN: the column; CONST: the constant
    const uint8_t* pc;       // HORNER: the constant; EMIT: the output member
};
static_assert(sizeof(GraphOp) == 40, "ten dwords, fetched uniformly");

// Every address in a resolved op is device memory: the column and output accesses are told so, since
// the generic (flat) form of a pointer read out of a struct also counts against the LDS counter and
// would serialise with the slot traffic; a constant sits at a uniform address nothing writes during
// the launch, so its eight words come through the scalar cache
typedef uint32_t graph_u32x4 __attribute__((ext_vector_type(4)));  // a plain vector: no constructor takes its address
MBLS_DEV Fr load_column(const uint8_t* p) {
    typedef __attribute__((address_space(1))) const graph_u32x4 global_u4;
    const global_u4* q = (const global_u4*)p;
    const graph_u32x4 x = q[0], y = q[1];
    Fr r;
    r.v[0] = x.x, r.v[1] = x.y, r.v[2] = x.z, r.v[3] = x.w, r.v[4] = y.x, r.v[5] = y.y, r.v[6] = y.z, r.v[7] = y.w;
    return r;
}
MBLS_DEV Fr load_constant(const uint8_t* p) {
    typedef __attribute__((address_space(4))) const graph_u32x4 constant_u4;
    const constant_u4* q = (const constant_u4*)p;
    const graph_u32x4 x = q[0], y = q[1];
    Fr r;
    r.v[0] = x.x, r.v[1] = x.y, r.v[2] = x.z, r.v[3] = x.w, r.v[4] = y.x, r.v[5] = y.y, r.v[6] = y.z, r.v[7] = y.w;
    return r;
}
MBLS_DEV void store_output(uint8_t* p, const Fr& a) {
    typedef __attribute__((address_space(1))) graph_u32x4 global_u4;
    global_u4* q = (global_u4*)p;
    q[0] = graph_u32x4{a.v[0], a.v[1], a.v[2], a.v[3]};
    q[1] = graph_u32x4{a.v[4], a.v[5], a.v[6], a.v[7]};
}

// one operand; `from` is uniform, and never GRAPH_FROM_NONE here
MBLS_DEV Fr graph_operand(uint32_t from, uint32_t slot, uint32_t off, const uint8_t* p, const Fr& prev,
                          const uint32_t* sh, uint32_t i, uint32_t size) {
    switch (from) {
    case GRAPH_FROM_PREV:
        return prev;
    case GRAPH_FROM_SLOT:
        return slot_get<GRAPH_THREADS>(sh, slot);
    case GRAPH_FROM_COLUMN: {
        uint32_t j = i + off;  // < 2 size <= 2^27
        j -= j >= size ? size : 0;
        return load_column(p + 32 * (size_t)j);
    }
    default:  // GRAPH_FROM_CONST
        return load_constant(p);
    }
}

__global__ __launch_bounds__(GRAPH_THREADS) void k_graph(const GraphOp* __restrict__ ops, uint32_t n_ops, uint32_t size,
                                                         uint32_t tiles) {
    extern __shared__ __attribute__((aligned(16))) uint32_t graph_slots[];
    uint32_t* sh = graph_slots;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t row = tile * GRAPH_THREADS + threadIdx.x;
        const bool live = row < size;
        const uint32_t i = live ? row : size - 1;
        Fr prev = Fr::zero();
        for (uint32_t pc = 0; pc < n_ops; ++pc) {
            const GraphOp o = ops[pc];
            const uint32_t b_from = o.ctl >> 12 & 0xf;
            const Fr a = graph_operand(o.ctl >> 8 & 0xf, o.slots & 0xff, o.a_off, o.pa, prev, sh, i, size);
            Fr b = prev;
            if (b_from != GRAPH_FROM_NONE) b = graph_operand(b_from, o.slots >> 8 & 0xff, o.b_off, o.pb, prev, sh, i, size);
            Fr r;
            switch (o.ctl & 0xff) {
            case MBLS_GRAPH_ADD:
                r = a + b;
                break;
            case MBLS_GRAPH_SUB:
                r = a - b;
                break;
            case MBLS_GRAPH_MUL:
                r = a * b;
                break;
            case MBLS_GRAPH_SQUARE:
                r = sqr(a);
                break;
            case MBLS_GRAPH_DOUBLE:
                r = dbl(a);
                break;
            case MBLS_GRAPH_NEG:
                r = neg(a);
                break;
            case MBLS_GRAPH_HORNER:
                r = a * load_constant(o.pc) + b;
                break;
            case MBLS_GRAPH_STORE:
                r = a;
                break;
            default:  // MBLS_GRAPH_EMIT: the host admits no other opcode.  It defines no value
                if (live) store_output(const_cast<uint8_t*>(o.pc) + 32 * (size_t)row, a);
                continue;
            }
            if (o.ctl >> 16 & 1) slot_put<GRAPH_THREADS>(sh, o.slots >> 16 & 0xff, r);
            prev = r;
        }
    }
}

// the evaluator's parts of the eval entry (rowprog_eval): mbls_graph.hpp's rules and slot
// assignment, and an op resolved with its placement
struct GraphEval {
    using Src = mbls_fr_graph_op;
    using Op = GraphOp;
    static constexpr int THREADS = GRAPH_THREADS, MAX_GRID = GRAPH_MAX_GRID, MAX_COLUMNS = GRAPH_MAX_COLUMNS;
    static constexpr auto kernel = k_graph;
    GraphInfo info;
    const GraphPlaced* placed;

    eIcicleError check(const Src* prog, int n_ops, int n_columns, int n_constants, int n_outputs) {
        static thread_local std::vector<GraphPlaced> buf;  // the thread's own, reused by its next call
        const eIcicleError er = graph_check(prog, n_ops, n_columns, n_constants, n_outputs, &info, &buf);
        placed = buf.data();
        return er;
    }
    size_t lds() const { return GRAPH_SLOT_BYTES * (size_t)info.peak; }  // <= 64 KiB
    Op resolve(int k, const Src& o, const RowProgAddr& at) const {
        const GraphPlaced& p = placed[k];
        Op q;
        q.ctl = (uint32_t)p.op | (uint32_t)p.a_from << 8 | (uint32_t)p.b_from << 12 | (uint32_t)p.put << 16;
        q.slots = (uint32_t)p.a_slot | (uint32_t)p.b_slot << 8 | (uint32_t)p.put_slot << 16;
        const mbls_fr_graph_src* src[2] = {&o.a, &o.b};
        uint32_t off[2] = {0, 0};
        const uint8_t* ptr[2] = {nullptr, nullptr};
        for (int s = 0; s < 2; ++s) {
            const mbls_fr_graph_src& v = *src[s];
            if (v.kind == MBLS_GRAPH_COLUMN) {
                off[s] = rowprog_offset(v.rot, at.rot_stride, at.size);
                ptr[s] = at.columns[v.idx];
            } else if (v.kind == MBLS_GRAPH_CONST) {
                ptr[s] = at.constants + 32 * (size_t)v.idx;
            }
        }
        q.a_off = off[0], q.b_off = off[1], q.pa = ptr[0], q.pb = ptr[1];
        q.pc =o.op == MBLS_GRAPH_HORNER ? at.constants + 32 * (size_t)o.c
               : o.op == MBLS_GRAPH_EMIT ? at.output + at.col_bytes * (size_t)o.c
                                         : nullptr;
        return q;
    }
};

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError mbls_fr_graph_check(const mbls_fr_graph_op* program, int n_ops, int n_columns, int n_constants, int n_outputs,
                                 int32_t* out) {
    if (!program || !out) return MBLS_INVALID_POINTER;
    GraphInfo info = {-1, 0, 0, 0, 0, 0, 0};
    const eIcicleError er = graph_check(program, n_ops, n_columns, n_constants, n_outputs, &info);
    if (info.peak < 0) return er;  // refused by another rule than the budget: nothing to report
    out[0] = info.peak;
    out[1] = info.peak_at;
    out[2] = info.resident;
    out[3] = info.forwarded;
    out[4] = info.loads;
    out[5] = info.pairs;
    out[6] = info.muls;
    out[7] = GRAPH_BUDGET;
    return er;
}

eIcicleError mbls_fr_eval_graph(const mbls_fr_t* const* columns, int n_columns, size_t size, size_t rot_stride,
                                const mbls_fr_t* constants, int n_constants, const mbls_fr_graph_op* program, int n_ops,
                                int n_outputs, const VecOpsConfig* config, mbls_fr_t* output) {
    return rowprog_eval<GraphEval>(columns, n_columns, size, rot_stride, constants, n_constants, program, n_ops, n_outputs,
                                   config, output);
}

}  // extern "C"
