// graph_host.cpp -- stand-alone driver of the graph evaluator's host lowering (csrc/mbls_graph.hpp:
// validation, lifetimes, slot assignment) with no device and no HIP, so that it builds with g++
// and runs under -fsanitize=address,undefined (tests/test_graph_abi.py).
//
// stdin: any number of cases, each "n_ops n_columns n_constants n_outputs" and then n_ops ops of 8
// integers (op, a.kind, a.idx, a.rot, b.kind, b.idx, b.rot, c).  stdout, per case: one line with
// the error code and, where they were written, the seven numbers of GraphInfo and the budget; for
// an accepted program a second line with, per op, the slot its result is written to (-1: none) and
// a third with where its operands come from, "<a_from><b_from>" as GraphFrom digits, a slot in
// brackets behind a digit 2.  The driver also replays the placement: a slot is written only while
// free, read only while it holds the value the program names, and its index stays below the peak.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mbls_graph.hpp"

using namespace mbls;

static int fail(const char* what, int k) {
    std::fprintf(stderr, "placement: %s at op %d\n", what, k);
    return 1;
}

static int replay(const std::vector<mbls_fr_graph_op>& prog, const std::vector<GraphPlaced>& placed, const GraphInfo& info) {
    const int n = (int)prog.size();
    std::vector<int> last((size_t)n, -1), holds(GRAPH_BUDGET, -1);  // holds[s]: the value in slot s, -1 free
    for (int k = 0; k < n; ++k) {
        if (prog[(size_t)k].a.kind == MBLS_GRAPH_VALUE) last[(size_t)prog[(size_t)k].a.idx] = k;
        if (prog[(size_t)k].b.kind == MBLS_GRAPH_VALUE) last[(size_t)prog[(size_t)k].b.idx] = k;
    }
    for (int k = 0; k < n; ++k) {
        const mbls_fr_graph_op& o = prog[(size_t)k];
        const GraphPlaced& p = placed[(size_t)k];
        const mbls_fr_graph_src* src[2] = {&o.a, &o.b};
        const int from[2] = {p.a_from, p.b_from}, at[2] = {p.a_slot, p.b_slot};
        if (p.op != o.op) return fail("opcode", k);
        for (int s = 0; s < 2; ++s) {
            const mbls_fr_graph_src& v = *src[s];
            const int want = v.kind == MBLS_GRAPH_NONE     ? GRAPH_FROM_NONE
                             : v.kind == MBLS_GRAPH_COLUMN ? GRAPH_FROM_COLUMN
                             : v.kind == MBLS_GRAPH_CONST  ? GRAPH_FROM_CONST
                             : v.idx == k - 1              ? GRAPH_FROM_PREV
                                                           : GRAPH_FROM_SLOT;
            if (from[s] != want) return fail("operand source", k);
            if (want == GRAPH_FROM_SLOT && (at[s] >= info.peak || holds[(size_t)at[s]] != v.idx)) return fail("slot read", k);
        }
        for (int s = 0; s < GRAPH_BUDGET; ++s)
            if (holds[(size_t)s] >= 0 && last[(size_t)holds[(size_t)s]] == k) holds[(size_t)s] = -1;
        const bool resident = last[(size_t)k] > k + 1;
        if ((p.put != 0) != resident) return fail("put flag", k);
        if (resident) {
            if (p.put_slot >= info.peak || holds[p.put_slot] >= 0) return fail("slot write", k);
            for (int s = 0; s < p.put_slot; ++s)
                if (holds[(size_t)s] < 0) return fail("not the lowest free slot", k);
            holds[p.put_slot] = k;
        }
    }
    return 0;
}

int main() {
    int n_ops, n_columns, n_constants, n_outputs;
    while (std::scanf("%d %d %d %d", &n_ops, &n_columns, &n_constants, &n_outputs) == 4) {
        if (n_ops < 0 || n_ops > (1 << 20)) return 2;
        std::vector<mbls_fr_graph_op> prog((size_t)n_ops);
        for (mbls_fr_graph_op& o : prog)
            if (std::scanf("%d %d %d %d %d %d %d %d", &o.op, &o.a.kind, &o.a.idx, &o.a.rot, &o.b.kind, &o.b.idx, &o.b.rot,
                           &o.c) != 8)
                return 2;
        GraphInfo info = {-1, 0, 0, 0, 0, 0, 0};
        std::vector<GraphPlaced> placed;
        // the vector's storage is exactly n_ops ops: a read past either end is the sanitizer's to report
        const eIcicleError er = graph_check(prog.data(), n_ops, n_columns, n_constants, n_outputs, &info, &placed);
        std::printf("%d", (int)er);
        if (info.peak >= 0)
            std::printf(" %d %d %d %d %d %d %d %d", info.peak, info.peak_at, info.resident, info.forwarded, info.loads,
                        info.pairs, info.muls, GRAPH_BUDGET);
        std::printf("\n");
        if (er != MBLS_SUCCESS) continue;
        if ((int)placed.size() != n_ops) return fail("size", 0);
        if (replay(prog, placed, info)) return 1;
        for (const GraphPlaced& p : placed) std::printf("%d ", p.put ? (int)p.put_slot : -1);
        std::printf("\n");
        for (const GraphPlaced& p : placed) {
            std::printf("%d", (int)p.a_from);
            if (p.a_from == GRAPH_FROM_SLOT) std::printf("[%d]", (int)p.a_slot);
            std::printf("%d", (int)p.b_from);
            if (p.b_from == GRAPH_FROM_SLOT) std::printf("[%d]", (int)p.b_slot);
            std::printf(" ");
        }
        std::printf("\n");
    }
    return 0;
}
