#!/usr/bin/env python3
"""Graph evaluator timing (device events on one stream, device-resident operands) at 2^22 rows, three
comparisons, every leg from the same tree and process:

  permutation   the two-output permutation factors for m = 3: mbls_fr_eval_graph on
                graph_model.permutation(3) and on from_stack() of the stack program, against
                mbls_fr_eval_program on the stack program
  shared        graph_model.shared_gates(6, 8), whose shared subexpression is computed once, against
                mbls_fr_eval_program on the stack program that recomputes it per constraint
  budget        graph_model.at_budget(B), every slot of the budget B in use, against the graph of the
                same values, op count and products whose peak is 4

The outputs of the legs of one comparison are compared for equality before the timing (the two
budget graphs, which fold in different orders, each against the Python model on a few rows).  One
warm-up round, then --reps rounds of --iters back-to-back calls per leg, the legs alternating;
prints the median, min and max time per call beside the ops, products and loads per row and the
peak.  There is no pass / fail bound.  --out FILE also writes the lines there.  MBLS_LIB selects
another in-tree build."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=22)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "midnight-bls12-381-cuda_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import bls12_381_amd as amd
    import expr_model as E
    import graph_model as G

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {amd.lib().mbls_version().decode()} lib {os.path.relpath(amd.LIB_PATH, ROOT)} "
        f"device {torch.cuda.get_device_name(0)}")
    n = 1 << a.logn
    pool = []  # columns are made once and shared by the comparisons

    def columns(k):
        while len(pool) < k:
            c = amd.torch_u64((n, 4))
            amd.gen_scalars(c, 0x6A0 + len(pool), montgomery=True)
            pool.append(c)
        return pool[:k]

    consts = amd.torch_u64((8, 4))
    amd.gen_scalars(consts, 0x6AF, montgomery=True)

    def graph_leg(prog, ncol, ncon, nout):
        info = amd.graph_check(prog, ncol, ncon, nout)
        out = amd.torch_u64((nout * n, 4))
        fn = lambda: amd.eval_graph(columns(ncol), prog, constants=consts[:ncon] if ncon else None, n_outputs=nout, out=out,
                                    is_async=True)
        what = (f"graph, {len(prog)} ops, {info['muls']} products, {info['loads']} loads, peak {info['peak']}, "
                f"{info['resident']} resident, {info['forwarded']} forwarded")
        return fn, out, what

    def stack_leg(prog, ncol, ncon, nout):
        info = amd.expr_check(prog, ncol, ncon, nout)
        out = amd.torch_u64((nout * n, 4))
        fn = lambda: amd.eval_program(columns(ncol), prog, constants=consts[:ncon] if ncon else None, n_outputs=nout, out=out,
                                      is_async=True)
        return fn, out, f"stack, {len(prog)} ops, {info['muls']} products, {info['loads']} loads, depth {info['depth']}"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    def compare(title, legs, same_function=True):
        outs = []
        for name, (fn, out, what) in legs.items():
            fn()
            outs.append(out)
        torch.cuda.synchronize()
        if same_function:
            assert all(torch.equal(outs[0], o) for o in outs[1:]), f"{title}: the legs' outputs differ"
            say(f"# {title}: the outputs of {', '.join(legs)} are equal")
        ts = {k: [] for k in legs}
        for rep in range(a.reps + 1):  # round 0 is the warm-up
            for k, (fn, _, _) in legs.items():
                t = timed(fn)
                if rep:
                    ts[k].append(t)
        med = {}
        for k, v in ts.items():
            v.sort()
            med[k] = v[len(v) // 2]
            say(f"{title} 2^{a.logn} {k}: median {med[k]:.4f} ms min {v[0]:.4f} max {v[-1]:.4f} per call ({legs[k][2]})")
        first = next(iter(legs))
        say(f"{title} 2^{a.logn} " + ", ".join(f"{k} / {first} {med[k] / med[first]:.3f}" for k in legs if k != first))

    m = 3
    compare("permutation", {"stack": stack_leg(E.permutation(m), 2 * m + 1, m + 2, 2),
                            "graph": graph_leg(G.permutation(m), 2 * m + 1, m + 2, 2),
                            "graph_from_stack": graph_leg(G.from_stack(E.permutation(m)), 2 * m + 1, m + 2, 2)})
    ns, nc = 6, 8
    compare("shared", {"stack": stack_leg(G.shared_gates_stack(ns, nc), ns + 1 + nc, 1, 1),
                       "graph": graph_leg(G.shared_gates(ns, nc), ns + 1 + nc, 1, 1)})
    budget = amd.graph_check(G.at_budget(1), 4, 0, 1)["budget"]
    # the two graphs fold the same values in another order, which SUB and MUL do not commute over: each is
    # held against the Python model on 333 rows instead of against the other
    small = [amd.torch_u64((333, 4)) for _ in range(4)]
    for k, c in enumerate(small):
        amd.gen_scalars(c, 0x6B0 + k, montgomery=True)
    as_ints = lambda t: [int.from_bytes(bytes(r), "little") for r in amd.to_numpy_u64(t).view("u1").reshape(-1, 32)]
    for prog in (G.at_budget(4, budget), G.at_budget(budget)):
        assert as_ints(amd.eval_graph(small, prog)) == G.run([as_ints(c) for c in small], prog)[0], "budget: not the model's"
    say("# budget: both graphs equal the model on 333 rows")
    compare("budget", {"peak_4": graph_leg(G.at_budget(4, budget), 4, 0, 1),
                       f"peak_{budget}": graph_leg(G.at_budget(budget), 4, 0, 1)}, same_function=False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
