// mbls_graph.hpp -- host side of the Fr graph evaluator (csrc/graph.hip, mbls_fr_eval_graph): the
// validation, the lifetimes and the slot assignment.  Plain C++ with no device code and no HIP
// header, so a stand-alone program (tests/graph_host.cpp) runs it under the host sanitizers.
//
// A program is a list of three-address ops; op k defines value k (single assignment).  Value j is
// read for the last time by op last(j).  A read by op j + 1 is forwarded: it comes from the register
// that still holds the result of op j.  Value j is resident iff last(j) > j + 1, and then occupies
// one slot of the workgroup's LDS while ops j + 1 .. last(j) run.  The peak is the largest number of
// values resident during one op; the slot file has GRAPH_BUDGET slots.
//
// Slots are assigned by a linear scan in program order, lowest free slot first.  Op k loads its
// operands, then the slots of the values it reads last are freed, then its own result takes a slot
// (possibly one just freed).  Lifetimes are intervals on a line, so the scan never uses a slot index
// at or above the peak: the LDS a launch needs is peak slots.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "bls12_381_mi355x.h"

namespace mbls {

static constexpr int GRAPH_MAX_OPS = 16384, GRAPH_MAX_COLUMNS = 1024, GRAPH_MAX_CONSTANTS = 1024;
static constexpr int GRAPH_MAX_OUTPUTS = 8;
static constexpr int GRAPH_BUDGET = 32;  // resident values: 32 slots of 2 KiB are the 64 KiB of one workgroup

// where the kernel finds an operand
enum GraphFrom : uint32_t { GRAPH_FROM_NONE = 0, GRAPH_FROM_PREV, GRAPH_FROM_SLOT, GRAPH_FROM_COLUMN, GRAPH_FROM_CONST };

struct GraphInfo {
    int32_t peak, peak_at, resident, forwarded, loads, pairs, muls;
};

// one op after the scan: the opcode, where each operand comes from (the slot for GRAPH_FROM_SLOT)
// and whether the result is also written to a slot, and to which
struct GraphPlaced {
    uint8_t op, a_from, b_from, put;
    uint8_t a_slot, b_slot, put_slot;
};

static inline bool graph_is_binary(int32_t op) {
    return op == MBLS_GRAPH_ADD || op == MBLS_GRAPH_SUB || op == MBLS_GRAPH_MUL || op == MBLS_GRAPH_HORNER;
}

// The program rules.  INVALID_ARGUMENT for a count outside its limit, an unknown opcode or source
// kind, a `b` on a unary op, STORE or EMIT, NONE where an operand is needed, a VALUE that is not an
// earlier op or names an EMIT, a column, constant or output index out of range, an output emitted
// twice or never, a peak above GRAPH_BUDGET.  When only the peak is at fault *info is written all
// the same: peak_at is where a caller cuts the program.  `placed`, when given, receives the slot
// assignment of a program that passes.
static inline eIcicleError graph_check(const mbls_fr_graph_op* prog, int n_ops, int n_columns, int n_constants,
                                       int n_outputs, GraphInfo* info, std::vector<GraphPlaced>* placed = nullptr) {
    if (n_ops < 1 || n_ops > GRAPH_MAX_OPS || n_columns < 1 || n_columns > GRAPH_MAX_COLUMNS || n_constants < 0 ||
        n_constants > GRAPH_MAX_CONSTANTS || n_outputs < 1 || n_outputs > GRAPH_MAX_OUTPUTS)
        return MBLS_INVALID_ARGUMENT;
    GraphInfo r = {0, 0, 0, 0, 0, 0, 0};
    std::vector<int32_t> last((size_t)n_ops, -1);  // last(j), -1 for a value nobody reads
    std::vector<std::pair<int32_t, int32_t>> reads;
    int emitted = 0;
    for (int k = 0; k < n_ops; ++k) {
        const mbls_fr_graph_op& o = prog[k];
        if (o.op < MBLS_GRAPH_ADD || o.op > MBLS_GRAPH_EMIT) return MBLS_INVALID_ARGUMENT;
        const mbls_fr_graph_src* src[2] = {&o.a, &o.b};
        for (int s = 0; s < 2; ++s) {
            const mbls_fr_graph_src& v = *src[s];
            const bool needed = s == 0 || graph_is_binary(o.op);
            if (v.kind < MBLS_GRAPH_NONE || v.kind > MBLS_GRAPH_CONST) return MBLS_INVALID_ARGUMENT;
            if ((v.kind == MBLS_GRAPH_NONE) == needed) return MBLS_INVALID_ARGUMENT;
            switch (v.kind) {
            case MBLS_GRAPH_VALUE:
                if (v.idx < 0 || v.idx >= k || prog[v.idx].op == MBLS_GRAPH_EMIT) return MBLS_INVALID_ARGUMENT;
                last[(size_t)v.idx] = k;
                r.forwarded += v.idx == k - 1;
                break;
            case MBLS_GRAPH_COLUMN:
                if (v.idx < 0 || v.idx >= n_columns) return MBLS_INVALID_ARGUMENT;
                reads.emplace_back(v.idx, v.rot);
                ++r.loads;
                break;
            case MBLS_GRAPH_CONST:
                if (v.idx < 0 || v.idx >= n_constants) return MBLS_INVALID_ARGUMENT;
                break;
            default:
                break;
            }
        }
        if (o.op == MBLS_GRAPH_HORNER && (o.c < 0 || o.c >= n_constants)) return MBLS_INVALID_ARGUMENT;
        if (o.op == MBLS_GRAPH_EMIT) {
            if (o.c < 0 || o.c >= n_outputs || (emitted >> o.c & 1)) return MBLS_INVALID_ARGUMENT;
            emitted |= 1 << o.c;
        }
        r.muls += o.op == MBLS_GRAPH_MUL || o.op == MBLS_GRAPH_SQUARE || o.op == MBLS_GRAPH_HORNER;
    }
    if (emitted != (1 << n_outputs) - 1) return MBLS_INVALID_ARGUMENT;
    std::sort(reads.begin(), reads.end());
    r.pairs = (int32_t)(std::unique(reads.begin(), reads.end()) - reads.begin());

    // the residents of op k are the values j with j + 1 <= k <= last(j) and last(j) > j + 1
    std::vector<int32_t> ends((size_t)n_ops + 1, 0);  // ends[k]: residents whose last read is op k - 1
    int live = 0;
    for (int k = 0; k < n_ops; ++k) {
        live -= ends[(size_t)k];
        if (k > 0 && last[(size_t)k - 1] > k) {
            ++live, ++r.resident;
            ++ends[(size_t)last[(size_t)k - 1] + 1];
        }
        if (live > r.peak) r.peak = live, r.peak_at = k;
    }
    *info = r;
    if (r.peak > GRAPH_BUDGET) return MBLS_INVALID_ARGUMENT;
    if (!placed) return MBLS_SUCCESS;

    // the linear scan; r.peak <= GRAPH_BUDGET <= 32, so a 32-bit mask holds the free slots
    placed->assign((size_t)n_ops, GraphPlaced{});
    std::vector<uint8_t> slot((size_t)n_ops, 0);
    uint32_t used = 0;
    for (int k = 0; k < n_ops; ++k) {
        const mbls_fr_graph_op& o = prog[k];
        GraphPlaced& q = (*placed)[(size_t)k];
        q.op = (uint8_t)o.op;
        const mbls_fr_graph_src* src[2] = {&o.a, &o.b};
        uint8_t from[2] = {GRAPH_FROM_NONE, GRAPH_FROM_NONE}, at[2] = {0, 0};
        for (int s = 0; s < 2; ++s) {
            const mbls_fr_graph_src& v = *src[s];
            if (v.kind == MBLS_GRAPH_VALUE) {
                from[s] = v.idx == k - 1 ? GRAPH_FROM_PREV : GRAPH_FROM_SLOT;
                at[s] = slot[(size_t)v.idx];
            } else if (v.kind == MBLS_GRAPH_COLUMN) {
                from[s] = GRAPH_FROM_COLUMN;
            } else if (v.kind == MBLS_GRAPH_CONST) {
                from[s] = GRAPH_FROM_CONST;
            }
        }
        // the operands are loaded: free what this op reads last (a forwarded read frees nothing
        // unless the value is resident for a later reader, and then this is not its last read)
        for (int s = 0; s < 2; ++s) {
            const mbls_fr_graph_src& v = *src[s];
            if (v.kind == MBLS_GRAPH_VALUE && last[(size_t)v.idx] == k && k > v.idx + 1) used &= ~(1u << slot[(size_t)v.idx]);
        }
        q.a_from = from[0], q.b_from = from[1], q.a_slot = at[0], q.b_slot = at[1];
        if (last[(size_t)k] > k + 1) {
            int f = 0;
            while (used >> f & 1) ++f;  // f < peak <= 32: fewer than peak values are resident here
            used |= 1u << f;
            slot[(size_t)k] = (uint8_t)f;
            q.put = 1, q.put_slot = (uint8_t)f;
        }
    }
    return MBLS_SUCCESS;
}

}  // namespace mbls
