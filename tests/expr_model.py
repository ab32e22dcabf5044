"""Pure-Python model of the Fr expression evaluator (csrc/expr.hip, mbls_fr_eval_program): the
validator with the ABI's rules, the interpreter over big integers mod r, and builders of the programs
a prover runs -- the permutation numerator / denominator, the theta compression, a gate fold -- plus
a seeded generator of random valid programs.  Values are Montgomery-form integers, as the library's
elements are; a program is a list of (op, a, b) tuples."""
import random

import scan_model as S

R = S.R
mont = S.mont
mmul = S.mmul

(COLUMN, CONST, ADD, SUB, MUL, NEG, DOUBLE, SQUARE, SCALE, HORNER, EMIT) = range(11)
MAX_OPS, MAX_COLUMNS, MAX_CONSTANTS, MAX_OUTPUTS, MAX_DEPTH, MAX_ROWS = 4096, 1024, 1024, 8, 8, 1 << 26
# (pops, pushes)
ARITY = {COLUMN: (0, 1), CONST: (0, 1), ADD: (2, 1), SUB: (2, 1), MUL: (2, 1), NEG: (1, 1), DOUBLE: (1, 1),
         SQUARE: (1, 1), SCALE: (1, 1), HORNER: (2, 1), EMIT: (1, 0)}


class ProgramError(ValueError):
    """what the ABI answers with INVALID_ARGUMENT"""


def check(program, n_columns, n_constants, n_outputs):
    """the ABI's program rules; returns dict(depth, loads, muls, pairs) or raises ProgramError"""
    if not 1 <= len(program) <= MAX_OPS:
        raise ProgramError("n_ops")
    if not 1 <= n_columns <= MAX_COLUMNS:
        raise ProgramError("n_columns")
    if not 0 <= n_constants <= MAX_CONSTANTS:
        raise ProgramError("n_constants")
    if not 1 <= n_outputs <= MAX_OUTPUTS:
        raise ProgramError("n_outputs")
    depth = top = loads = muls = 0
    emitted, pairs = set(), set()
    for k, (op, a, b) in enumerate(program):
        if op not in ARITY:
            raise ProgramError(f"op {k}: opcode {op}")
        if op == COLUMN:
            if not 0 <= a < n_columns:
                raise ProgramError(f"op {k}: column {a}")
            loads += 1
            pairs.add((a, b))
        if op in (CONST, SCALE, HORNER) and not 0 <= a < n_constants:
            raise ProgramError(f"op {k}: constant {a}")
        if op == EMIT:
            if not 0 <= a < n_outputs:
                raise ProgramError(f"op {k}: output {a}")
            if a in emitted:
                raise ProgramError(f"op {k}: output {a} emitted twice")
            emitted.add(a)
        muls += op in (MUL, SQUARE, SCALE, HORNER)
        pops, pushes = ARITY[op]
        if depth < pops:
            raise ProgramError(f"op {k}: pop from an empty stack")
        depth += pushes - pops
        if depth > MAX_DEPTH:
            raise ProgramError(f"op {k}: depth {depth}")
        top = max(top, depth)
    if depth:
        raise ProgramError("stack not empty at the end")
    if len(emitted) != n_outputs:
        raise ProgramError("an output is never emitted")
    return dict(depth=top, loads=loads, muls=muls, pairs=len(pairs))


def run(columns, program, constants=(), n_outputs=1, rot_stride=1):
    """outputs[k][i], by the ABI's semantics, after check()"""
    check(program, len(columns), len(constants), n_outputs)
    size = len(columns[0])
    if not 1 <= size <= MAX_ROWS or not 1 <= rot_stride <= MAX_ROWS or any(len(c) != size for c in columns):
        raise ProgramError("size")
    out = [[None] * size for _ in range(n_outputs)]
    for i in range(size):
        st = []
        for op, a, b in program:
            if op == COLUMN:
                st.append(columns[a][(i + b * rot_stride) % size])
            elif op == CONST:
                st.append(constants[a])
            elif op in (ADD, SUB, MUL):
                y, x = st.pop(), st.pop()
                st.append((x + y) % R if op == ADD else (x - y) % R if op == SUB else mmul(x, y))
            elif op == NEG:
                st[-1] = -st[-1] % R
            elif op == DOUBLE:
                st[-1] = 2 * st[-1] % R
            elif op == SQUARE:
                st[-1] = mmul(st[-1], st[-1])
            elif op == SCALE:
                st[-1] = mmul(st[-1], constants[a])
            elif op == HORNER:
                t, acc = st.pop(), st.pop()
                st.append((mmul(acc, constants[a]) + t) % R)
            else:
                out[a][i] = st.pop()
    return out


# ----------------------------------------------------------------------------- builders
def permutation(m):
    """Columns v_0 .. v_{m-1}, sigma_0 .. sigma_{m-1}, X (2 m + 1 of them); constants beta delta^0 ..
    beta delta^{m-1}, beta, gamma (m + 2).  Output 0 = prod_k (v_k + beta delta^k X + gamma), output 1 =
    prod_k (v_k + beta sigma_k + gamma): the factors of the permutation grand product."""
    prog = []
    for side in range(2):
        for k in range(m):
            prog += [(COLUMN, 2 * m, 0), (SCALE, k, 0)] if side == 0 else [(COLUMN, m + k, 0), (SCALE, m, 0)]
            prog += [(COLUMN, k, 0), (ADD, 0, 0), (CONST, m + 1, 0), (ADD, 0, 0)]
            if k:
                prog.append((MUL, 0, 0))
        prog.append((EMIT, side, 0))
    return prog


def compression(m):
    """sum_k theta^k a_k over columns a_0 .. a_{m-1}, constants [theta]: Horner from the top column"""
    prog = [(COLUMN, m - 1, 0)]
    for k in range(m - 2, -1, -1):
        prog += [(COLUMN, k, 0), (HORNER, 0, 0)]
    return prog + [(EMIT, 0, 0)]


def gates():
    """the constraints of gate_fold over columns q, a, b, c: q (a b - c) with b read one row ahead,
    q (a - c) with c read one row back, a^2 - a"""
    return [[(COLUMN, 0, 0), (COLUMN, 1, 0), (COLUMN, 2, 1), (MUL, 0, 0), (COLUMN, 3, 0), (SUB, 0, 0), (MUL, 0, 0)],
            [(COLUMN, 0, 0), (COLUMN, 1, 0), (COLUMN, 3, -1), (SUB, 0, 0), (MUL, 0, 0)],
            [(COLUMN, 1, 0), (SQUARE, 0, 0), (COLUMN, 1, 0), (SUB, 0, 0)]]


def gate_fold(horner=True):
    """h = ((g_0 y + g_1) y + g_2) y over gates(), constants [y]: the evaluate_h fold, with HORNER and
    SCALE, or the same arithmetic written with CONST, MUL and ADD"""
    g = gates()
    prog = list(g[0])
    for term in g[1:]:
        prog += term + [(HORNER, 0, 0)] if horner else [(CONST, 0, 0), (MUL, 0, 0)] + term + [(ADD, 0, 0)]
    prog += [(SCALE, 0, 0)] if horner else [(CONST, 0, 0), (MUL, 0, 0)]
    return prog + [(EMIT, 0, 0)]


def random_program(seed, n_ops, depth, n_columns, n_constants, n_outputs=1, max_rot=3):
    """a seeded valid program of exactly n_ops ops whose stack reaches exactly `depth` (<= MAX_DEPTH);
    n_constants >= 1"""
    assert 1 <= depth <= MAX_DEPTH and n_constants >= 1 and n_ops >= 2 * depth + 2 * n_outputs
    rnd = random.Random(seed)
    col = lambda: (COLUMN, rnd.randrange(n_columns), rnd.randint(-max_rot, max_rot))
    push = lambda: col() if rnd.random() < 0.7 else (CONST, rnd.randrange(n_constants), 0)
    unary = lambda: rnd.choice([(NEG, 0, 0), (DOUBLE, 0, 0), (SQUARE, 0, 0), (SCALE, rnd.randrange(n_constants), 0)])
    binary = lambda: rnd.choice([(ADD, 0, 0), (SUB, 0, 0), (MUL, 0, 0), (HORNER, rnd.randrange(n_constants), 0)])
    prog = [push() for _ in range(depth)]  # reach the target depth once, at the start
    d, left_out = depth, n_outputs  # d >= 1 throughout the body
    while True:
        # ops still needed to finish from here: fold to one element, emit it, then push + emit per further
        # output.  A binary op leaves the room as it is, a unary one takes 1, a push 2 (itself and its fold)
        room = n_ops - len(prog) - (d + 2 * (left_out - 1))
        assert room >= 0
        if room == 0:
            break
        kinds = ["unary"] + ["binary"] * (d >= 2) + ["push"] * (d < depth and room >= 2)
        kind = rnd.choice(kinds)
        if kind == "push":
            prog.append(push())
            d += 1
        elif kind == "binary":
            prog.append(binary())
            d -= 1
        else:
            prog.append(unary())
    order = list(range(n_outputs))
    rnd.shuffle(order)
    while left_out:
        if d == 0:
            prog.append(push())
            d = 1
        while d > 1:
            prog.append(binary())
            d -= 1
        prog.append((EMIT, order[n_outputs - left_out], 0))
        d, left_out = 0, left_out - 1
    assert len(prog) == n_ops, (len(prog), n_ops)
    return prog
