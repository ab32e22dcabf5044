// expr.hip -- Fr expression evaluator: one caller-supplied straight-line stack program run once per
// row over columns read at rotated rows (mbls_fr_eval_program).  It is what a halo2 prover does
// between the MSM / NTT / scan calls: the permutation numerators and denominators, the lookup
// compressions, the constraint folds of the quotient.  No reference counterpart: the reference
// composes these on the CPU.
//
// One launch.  A lane owns one row of a tile of 256 contiguous rows; a workgroup strides over the
// tiles.  The host validates the program by simulating its stack and resolves it into 16-byte ops
// in the scratch context: the opcode, the stack depth before the op, the row offset reduced into
// [0, size), and the one address the op needs (the column, the constant, the output member).  Every
// lane of a wave reads the same op, so the fetch is uniform and the dispatch is a uniform switch.
//
// The operand stack is never a register array (a dynamically indexed one would go to private
// memory).  Its top is a register value; the slots below live in LDS, word-major: word w of slot s
// of lane t at ((s * 8 + w) * 256 + t) * 4, so a wave's access to one word is 64 consecutive dwords.
// A lane only ever touches its own words: no barrier.  The depth before each op is a field of the
// resolved op, so the kernel carries no stack pointer.  The LDS is dynamic, (max depth - 1) slots
// of 8 KiB: a shallow program leaves room for more workgroups per CU.
//
// Columns are witness-derived: no branch and no address depends on a field value.  The conditions
// are on the program, the tile and the size.  Rows past the end of a partial tile compute on the
// last row and store nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "mbls_rowprog.hpp"

namespace mbls {

static constexpr int EXPR_THREADS = 256;
static constexpr int EXPR_MAX_OPS = 4096, EXPR_MAX_COLUMNS = 1024, EXPR_MAX_CONSTANTS = 1024;
static constexpr int EXPR_MAX_OUTPUTS = 8, EXPR_MAX_DEPTH = 8;
static constexpr size_t EXPR_SLOT_BYTES = 32 * (size_t)EXPR_THREADS;  // one stack slot of a workgroup
static constexpr int EXPR_MAX_GRID = 256 * 8;  // 8 workgroups per CU is the residency limit; stride beyond

// a resolved op: what the kernel reads
struct ExprOp {
    uint32_t op;     // mbls_fr_expr_opcode | depth before the op << 8
    uint32_t off;    // COLUMN: (b * rot_stride) mod size
    const uint8_t* p;  // COLUMN: the column; CONST, SCALE, HORNER: the constant; EMIT: the output member
};
static_assert(sizeof(ExprOp) == 16, "one 16-byte fetch per op");

__global__ __launch_bounds__(EXPR_THREADS) void k_expr(const ExprOp* __restrict__ ops, uint32_t n_ops, uint32_t size,
                                                       uint32_t tiles) {
    extern __shared__ __attribute__((aligned(16))) uint32_t expr_stack[];
    uint32_t* sh = expr_stack;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t row = tile * EXPR_THREADS + threadIdx.x;
        const bool live = row < size;
        const uint32_t i = live ? row : size - 1;
        Fr top = Fr::zero();
        for (uint32_t pc = 0; pc < n_ops; ++pc) {
            const ExprOp o = ops[pc];
            const uint32_t d = o.op >> 8;  // depth before the op: top is element d - 1, LDS holds 0 .. d - 2
            switch (o.op & 0xff) {
            case MBLS_EXPR_COLUMN: {
                uint32_t j = i + o.off;  // < 2 size <= 2^27
                j -= j >= size ? size : 0;
                if (d) slot_put<EXPR_THREADS>(sh, d - 1, top);
                top = load<FrCfg>(o.p + 32 * (size_t)j);
                break;
            }
            case MBLS_EXPR_CONST:
                if (d) slot_put<EXPR_THREADS>(sh, d - 1, top);
                top = load<FrCfg>(o.p);
                break;
            case MBLS_EXPR_ADD:
                top = slot_get<EXPR_THREADS>(sh, d - 2) + top;
                break;
            case MBLS_EXPR_SUB:
                top = slot_get<EXPR_THREADS>(sh, d - 2) - top;
                break;
            case MBLS_EXPR_MUL:
                top = slot_get<EXPR_THREADS>(sh, d - 2) * top;
                break;
            case MBLS_EXPR_NEG:
                top = neg(top);
                break;
            case MBLS_EXPR_DOUBLE:
                top = dbl(top);
                break;
            case MBLS_EXPR_SQUARE:
                top = sqr(top);
                break;
            case MBLS_EXPR_SCALE:
                top = top * load<FrCfg>(o.p);
                break;
            case MBLS_EXPR_HORNER:
                top = slot_get<EXPR_THREADS>(sh, d - 2) * load<FrCfg>(o.p) + top;
                break;
            default:  // MBLS_EXPR_EMIT: the host admits no other opcode
                if (live) store<FrCfg>(const_cast<uint8_t*>(o.p) + 32 * (size_t)row, top);
                if (d > 1) top = slot_get<EXPR_THREADS>(sh, d - 2);
                break;
            }
        }
    }
}

// ---- host side
struct ExprInfo {
    int32_t depth, loads, muls, pairs;
};

// The program rules, by simulating the stack: INVALID_ARGUMENT for a count outside its limit, an
// unknown opcode, an index out of range, a pop from an empty stack, a depth above EXPR_MAX_DEPTH, an
// output emitted twice or never, a stack that is not empty at the end.
static eIcicleError expr_check(const mbls_fr_expr_op* prog, int n_ops, int n_columns, int n_constants, int n_outputs,
                               ExprInfo* info) {
    if (n_ops < 1 || n_ops > EXPR_MAX_OPS || n_columns < 1 || n_columns > EXPR_MAX_COLUMNS || n_constants < 0 ||
        n_constants > EXPR_MAX_CONSTANTS || n_outputs < 1 || n_outputs > EXPR_MAX_OUTPUTS)
        return MBLS_INVALID_ARGUMENT;
    int d = 0, emitted = 0;
    ExprInfo r = {0, 0, 0, 0};
    std::vector<std::pair<int32_t, int32_t>> reads;
    for (int k = 0; k < n_ops; ++k) {
        const mbls_fr_expr_op& o = prog[k];
        int pops = 0, pushes = 0;
        switch (o.op) {
        case MBLS_EXPR_COLUMN:
            if (o.a < 0 || o.a >= n_columns) return MBLS_INVALID_ARGUMENT;
            reads.emplace_back(o.a, o.b);
            ++r.loads;
            pushes = 1;
            break;
        case MBLS_EXPR_CONST:
            if (o.a < 0 || o.a >= n_constants) return MBLS_INVALID_ARGUMENT;
            pushes = 1;
            break;
        case MBLS_EXPR_ADD:
        case MBLS_EXPR_SUB:
            pops = 2, pushes = 1;
            break;
        case MBLS_EXPR_MUL:
            ++r.muls;
            pops = 2, pushes = 1;
            break;
        case MBLS_EXPR_NEG:
        case MBLS_EXPR_DOUBLE:
            pops = 1, pushes = 1;
            break;
        case MBLS_EXPR_SQUARE:
            ++r.muls;
            pops = 1, pushes = 1;
            break;
        case MBLS_EXPR_SCALE:
            if (o.a < 0 || o.a >= n_constants) return MBLS_INVALID_ARGUMENT;
            ++r.muls;
            pops = 1, pushes = 1;
            break;
        case MBLS_EXPR_HORNER:
            if (o.a < 0 || o.a >= n_constants) return MBLS_INVALID_ARGUMENT;
            ++r.muls;
            pops = 2, pushes = 1;
            break;
        case MBLS_EXPR_EMIT:
            if (o.a < 0 || o.a >= n_outputs || (emitted >> o.a & 1)) return MBLS_INVALID_ARGUMENT;
            emitted |= 1 << o.a;
            pops = 1;
            break;
        default:
            return MBLS_INVALID_ARGUMENT;
        }
        if (d < pops) return MBLS_INVALID_ARGUMENT;
        d += pushes - pops;
        if (d > EXPR_MAX_DEPTH) return MBLS_INVALID_ARGUMENT;
        r.depth = std::max(r.depth, d);
    }
    if (d != 0 || emitted != (1 << n_outputs) - 1) return MBLS_INVALID_ARGUMENT;
    std::sort(reads.begin(), reads.end());
    r.pairs = (int32_t)(std::unique(reads.begin(), reads.end()) - reads.begin());
    *info = r;
    return MBLS_SUCCESS;
}

// the evaluator's parts of the eval entry (rowprog_eval): the stack simulation, and an op resolved
// with the depth the ops before it leave
struct ExprEval {
    using Src = mbls_fr_expr_op;
    using Op = ExprOp;
    static constexpr int THREADS = EXPR_THREADS, MAX_GRID = EXPR_MAX_GRID, MAX_COLUMNS = EXPR_MAX_COLUMNS;
    static constexpr auto kernel = k_expr;
    ExprInfo info;
    int d = 0;  // the depth before the next op to resolve

    eIcicleError check(const Src* prog, int n_ops, int n_columns, int n_constants, int n_outputs) {
        return expr_check(prog, n_ops, n_columns, n_constants, n_outputs, &info);
    }
    size_t lds() const { return EXPR_SLOT_BYTES * (size_t)(info.depth - 1); }  // <= 56 KiB
    Op resolve(int, const Src& o, const RowProgAddr& at) {
        Op q = {(uint32_t)o.op | (uint32_t)d << 8, 0, nullptr};
        switch (o.op) {
        case MBLS_EXPR_COLUMN:
            q.off = rowprog_offset(o.b, at.rot_stride, at.size);
            q.p = at.columns[o.a];
            ++d;
            break;
        case MBLS_EXPR_CONST:
            q.p = at.constants + 32 * (size_t)o.a;
            ++d;
            break;
        case MBLS_EXPR_SCALE:
            q.p = at.constants + 32 * (size_t)o.a;
            break;
        case MBLS_EXPR_HORNER:
            q.p = at.constants + 32 * (size_t)o.a;
            --d;
            break;
        case MBLS_EXPR_EMIT:
            q.p = at.output + at.col_bytes * (size_t)o.a;
            --d;
            break;
        case MBLS_EXPR_ADD:
        case MBLS_EXPR_SUB:
        case MBLS_EXPR_MUL:
            --d;
            break;
        default:  // NEG, DOUBLE, SQUARE: the depth stays
            break;
        }
        return q;
    }
};

}  // namespace mbls

using namespace mbls;

extern "C" {

eIcicleError mbls_fr_expr_check(const mbls_fr_expr_op* program, int n_ops, int n_columns, int n_constants, int n_outputs,
                                int32_t* out) {
    if (!program || !out) return MBLS_INVALID_POINTER;
    ExprInfo info;
    const eIcicleError er = expr_check(program, n_ops, n_columns, n_constants, n_outputs, &info);
    if (er != MBLS_SUCCESS) return er;
    out[0] = info.depth;
    out[1] = info.loads;
    out[2] = info.muls;
    out[3] = info.pairs;
    return MBLS_SUCCESS;
}

eIcicleError mbls_fr_eval_program(const mbls_fr_t* const* columns, int n_columns, size_t size, size_t rot_stride,
                                  const mbls_fr_t* constants, int n_constants, const mbls_fr_expr_op* program, int n_ops,
                                  int n_outputs, const VecOpsConfig* config, mbls_fr_t* output) {
    return rowprog_eval<ExprEval>(columns, n_columns, size, rot_stride, constants, n_constants, program, n_ops, n_outputs,
                                  config, output);
}

}  // extern "C"
