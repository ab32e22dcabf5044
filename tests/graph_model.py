"""Pure-Python model of the Fr graph evaluator (csrc/graph.hip, mbls_fr_eval_graph): the validator
with the ABI's rules and its eight residency numbers, the slot assignment of the host lowering, the
interpreter over big integers mod r, and builders -- any stack program of expr_model.py as a graph,
the permutation factors, a shared subexpression read by several constraints, a graph that fills the
slot file, and a seeded generator of random valid graphs.  Values are Montgomery-form integers, as
the library's elements are.  A program is a list of (op, a, b, c) tuples; a and b are sources,
(kind, idx, rot) triples; op k defines value k."""
import random

import expr_model as E

R = E.R
mont = E.mont
mmul = E.mmul
ProgramError = E.ProgramError  # what the ABI answers with INVALID_ARGUMENT

(ADD, SUB, MUL, SQUARE, DOUBLE, NEG, HORNER, STORE, EMIT) = range(9)
(NONE, VALUE, COLUMN, CONST) = range(4)
BINARY = (ADD, SUB, MUL, HORNER)
MAX_OPS, MAX_COLUMNS, MAX_CONSTANTS, MAX_OUTPUTS, MAX_ROWS, BUDGET = 16384, 1024, 1024, 8, 1 << 26, 32
FIELDS = ("peak", "peak_at", "resident", "forwarded", "loads", "pairs", "muls", "budget")

NO = (NONE, 0, 0)


def val(k):
    return (VALUE, k, 0)


def col(k, rot=0):
    return (COLUMN, k, rot)


def const(k):
    return (CONST, k, 0)


def last_reads(program):
    """last(j) for every value, None for one nobody reads"""
    last = [None] * len(program)
    for k, (op, a, b, c) in enumerate(program):
        for kind, idx, _ in (a, b):
            if kind == VALUE:
                last[idx] = k
    return last


def check(program, n_columns, n_constants, n_outputs):
    """the ABI's program rules; returns a dict of FIELDS or raises ProgramError.  A program refused
    only for its peak carries the dict as the exception's `info`."""
    if not 1 <= len(program) <= MAX_OPS:
        raise ProgramError("n_ops")
    if not 1 <= n_columns <= MAX_COLUMNS:
        raise ProgramError("n_columns")
    if not 0 <= n_constants <= MAX_CONSTANTS:
        raise ProgramError("n_constants")
    if not 1 <= n_outputs <= MAX_OUTPUTS:
        raise ProgramError("n_outputs")
    forwarded = loads = muls = 0
    emitted, pairs = set(), set()
    for k, (op, a, b, c) in enumerate(program):
        if op not in range(9):
            raise ProgramError(f"op {k}: opcode {op}")
        for name, (kind, idx, rot), needed in (("a", a, True), ("b", b, op in BINARY)):
            if kind not in range(4):
                raise ProgramError(f"op {k}: source kind {kind}")
            if (kind == NONE) == needed:
                raise ProgramError(f"op {k}: operand {name} " + ("missing" if needed else "not read by this opcode"))
            if kind == VALUE:
                if not 0 <= idx < k:
                    raise ProgramError(f"op {k}: value {idx}")
                if program[idx][0] == EMIT:
                    raise ProgramError(f"op {k}: value {idx} is an EMIT")
                forwarded += idx == k - 1
            if kind == COLUMN:
                if not 0 <= idx < n_columns:
                    raise ProgramError(f"op {k}: column {idx}")
                loads += 1
                pairs.add((idx, rot))
            if kind == CONST and not 0 <= idx < n_constants:
                raise ProgramError(f"op {k}: constant {idx}")
        if op == HORNER and not 0 <= c < n_constants:
            raise ProgramError(f"op {k}: constant {c}")
        if op == EMIT:
            if not 0 <= c < n_outputs:
                raise ProgramError(f"op {k}: output {c}")
            if c in emitted:
                raise ProgramError(f"op {k}: output {c} emitted twice")
            emitted.add(c)
        muls += op in (MUL, SQUARE, HORNER)
    if len(emitted) != n_outputs:
        raise ProgramError("an output is never emitted")
    last = last_reads(program)
    is_resident = [l is not None and l > j + 1 for j, l in enumerate(last)]
    # the definition, restated directly: value j is resident during ops j + 1 .. last(j)
    count = [0] * len(program)
    for j, l in enumerate(last):
        if is_resident[j]:
            for k in range(j + 1, l + 1):
                count[k] += 1
    peak = max(count)
    info = dict(peak=peak, peak_at=count.index(peak), resident=sum(is_resident), forwarded=forwarded, loads=loads,
                pairs=len(pairs), muls=muls, budget=BUDGET)
    if peak > BUDGET:
        err = ProgramError(f"peak {peak}")
        err.info = info
        raise err
    return info


def assign_slots(program):
    """the host lowering's linear scan, lowest free slot first: [slot or None per value].  Op k loads
    its operands, then the values it reads last leave their slots, then its own result takes one."""
    last = last_reads(program)
    slot, free_at = [None] * len(program), {}
    used = set()
    for k in range(len(program)):
        for j in free_at.pop(k, ()):
            used.discard(slot[j])
        if last[k] is not None and last[k] > k + 1:
            s = 0
            while s in used:
                s += 1
            used.add(s)
            slot[k] = s
            free_at.setdefault(last[k], []).append(k)
    return slot


def run(columns, program, constants=(), n_outputs=1, rot_stride=1):
    """outputs[k][i], by the ABI's semantics, after check()"""
    check(program, len(columns), len(constants), n_outputs)
    size = len(columns[0])
    if not 1 <= size <= MAX_ROWS or not 1 <= rot_stride <= MAX_ROWS or any(len(c) != size for c in columns):
        raise ProgramError("size")
    out = [[None] * size for _ in range(n_outputs)]
    for i in range(size):
        v = [None] * len(program)

        def get(src):
            kind, idx, rot = src
            return v[idx] if kind == VALUE else columns[idx][(i + rot * rot_stride) % size] if kind == COLUMN \
                else constants[idx]

        for k, (op, a, b, c) in enumerate(program):
            x = get(a)
            if op == ADD:
                v[k] = (x + get(b)) % R
            elif op == SUB:
                v[k] = (x - get(b)) % R
            elif op == MUL:
                v[k] = mmul(x, get(b))
            elif op == SQUARE:
                v[k] = mmul(x, x)
            elif op == DOUBLE:
                v[k] = 2 * x % R
            elif op == NEG:
                v[k] = -x % R
            elif op == HORNER:
                v[k] = (mmul(x, constants[c]) + get(b)) % R
            elif op == STORE:
                v[k] = x
            else:
                out[c][i] = x
    return out


# ----------------------------------------------------------------------------- builders
def from_stack(program):
    """a stack program of expr_model.py as a graph with the same outputs: a push becomes the source of
    the op that pops it, every other op one graph op (SCALE a MUL by a CONST source)"""
    st, g = [], []
    for op, a, b in program:
        if op == E.COLUMN:
            st.append(col(a, b))
            continue
        if op == E.CONST:
            st.append(const(a))
            continue
        if op == E.EMIT:
            g.append((EMIT, st.pop(), NO, a))
            continue
        if op in (E.ADD, E.SUB, E.MUL):
            y, x = st.pop(), st.pop()
            g.append(({E.ADD: ADD, E.SUB: SUB, E.MUL: MUL}[op], x, y, 0))
        elif op in (E.NEG, E.DOUBLE, E.SQUARE):
            g.append(({E.NEG: NEG, E.DOUBLE: DOUBLE, E.SQUARE: SQUARE}[op], st.pop(), NO, 0))
        elif op == E.SCALE:
            g.append((MUL, st.pop(), const(a), 0))
        else:  # HORNER: pop t, pop acc, push acc * constants[a] + t
            t, acc = st.pop(), st.pop()
            g.append((HORNER, acc, t, a))
        st.append(val(len(g) - 1))
    return g


def permutation(m):
    """the columns, constants and outputs of expr_model.permutation(m), three ops per factor: the
    HORNER v_k + (beta delta^k) X with both operands columns, + gamma, and the running product"""
    g = []
    for side in range(2):
        acc = None
        for k in range(m):
            g.append((HORNER, col(2 * m), col(k), k) if side == 0 else (HORNER, col(m + k), col(k), m))
            g.append((ADD, val(len(g) - 1), const(m + 1), 0))
            if acc is not None:
                g.append((MUL, val(len(g) - 1), val(acc), 0))
            acc = len(g) - 1
        g.append((EMIT, val(acc), NO, side))
    return g


def shared_gates(n_shared, n_constraints):
    """Columns s_0 .. s_{n_shared} and g_0 .. g_{n_constraints - 1}, constants [y].  S = s_0 s_1 .. is
    n_shared products, computed once; constraint j is S g_j with g_j read at rotation j mod 3 - 1; the
    output is the fold sum_j y^(n_constraints - 1 - j) S g_j, by HORNER."""
    g = [(MUL, col(0), col(1), 0)]
    for k in range(2, n_shared + 1):
        g.append((MUL, val(len(g) - 1), col(k), 0))
    s, h = len(g) - 1, None
    for j in range(n_constraints):
        g.append((MUL, val(s), col(n_shared + 1 + j, j % 3 - 1), 0))
        if h is not None:
            g.append((HORNER, val(h), val(len(g) - 1), 0))
        h = len(g) - 1
    return g + [(EMIT, val(h), NO, 0)]


def shared_gates_stack(n_shared, n_constraints):
    """the same output as a stack program of expr_model.py, which has to recompute S per constraint"""
    p = []
    for j in range(n_constraints):
        p += [(E.COLUMN, 0, 0)]
        for k in range(1, n_shared + 1):
            p += [(E.COLUMN, k, 0), (E.MUL, 0, 0)]
        p += [(E.COLUMN, n_shared + 1 + j, j % 3 - 1), (E.MUL, 0, 0)]
        if j:
            p.append((E.HORNER, 0, 0))
    return p + [(E.EMIT, 0, 0)]


AT_BUDGET_COLUMNS = 4


def at_budget(b, total=None):
    """A graph over AT_BUDGET_COLUMNS columns whose peak is exactly b >= 1, reached first at op b:
    `total` (default b) loaded values x_j = column j mod 4 at rotation j div 4, every one distinct, are
    folded into one accumulator, acc <- acc * x_j for even j and acc - x_j for odd j, which is not
    symmetric in the x_j, so two values that swap slots show.  They are loaded b at a time, last
    loaded first folded: while a group loads, the accumulator and all of the group but its last member,
    which is forwarded, hold a slot each.  2 total + 2 ops whatever b is: graphs of one `total` differ
    only in their peak."""
    total = b if total is None else total
    assert 1 <= b <= total
    load = lambda j: (STORE, col(j % AT_BUDGET_COLUMNS, j // AT_BUDGET_COLUMNS), NO, 0)
    g = [(STORE, col(0, -1), NO, 0)]  # the accumulator's start
    acc, done = 0, 0
    while done < total:
        n = min(b, total - done)
        first = len(g)
        g += [load(done + t) for t in range(n)]
        for t in range(n - 1, -1, -1):
            j = done + t
            g.append((MUL if j % 2 == 0 else SUB, val(acc), val(first + t), 0))
            acc = len(g) - 1
        done += n
    return g + [(EMIT, val(acc), NO, 0)]


def random_graph(seed, n_ops, n_columns, n_constants, n_outputs, max_rot, reach):
    """a seeded valid graph of exactly n_ops ops.  A VALUE source points at most `reach` ops back, so
    at most `reach` values are resident at once: reach <= BUDGET keeps the graph inside the budget."""
    assert n_ops >= 2 * n_outputs and reach >= 1
    rnd = random.Random(seed)
    emit_at = sorted(rnd.sample(range(1, n_ops - 1), n_outputs - 1)) + [n_ops - 1]
    order = list(range(n_outputs))
    rnd.shuffle(order)
    g = []

    def source(k):
        back = [j for j in range(max(0, k - reach), k) if g[j][0] != EMIT]
        t = rnd.random()
        if back and t < 0.55:
            # half of the VALUE sources are the previous op when it defines a value: forwarding
            return val(back[-1] if rnd.random() < 0.5 else rnd.choice(back))
        if n_constants and t > 0.9:
            return const(rnd.randrange(n_constants))
        return col(rnd.randrange(n_columns), rnd.randint(-max_rot, max_rot))

    for k in range(n_ops):
        if k in emit_at:
            g.append((EMIT, source(k), NO, order[emit_at.index(k)]))
            continue
        op = rnd.choice([ADD, SUB, MUL, SQUARE, DOUBLE, NEG, STORE] + [HORNER] * (n_constants > 0))
        g.append((op, source(k), source(k) if op in BINARY else NO, rnd.randrange(n_constants) if op == HORNER else 0))
    return g
