"""Directed operands for the saturated 32-bit-limb field arithmetic (tests/test_gpu_field.py).

Every list is generated from a fixed seed.  A case is a dict with the operands as Python integers
(`a`, `b`, ...), a `cls` (the side of the wave-uniform branch the case takes, or its operand class:
what the grouped / interleaved orders are built from) and a `tag` naming why it is there;
`tag == "random"` marks filler that no coverage condition may count.

The per-limb model (stage_gp, live_runs, ripple) restates what the row arithmetic's ballots see:
generate / propagate bits per 32-bit limb of the four carry chains of csrc/mbls_rowfield.hpp --
the addition a + b, the reduction t - m, the subtraction a - b and its + m correction."""
import random

MASK = 0xffffffff


class Field:
    def __init__(self, name, m, n):
        self.name, self.m, self.N = name, m, n
        self.R = 1 << (32 * n)
        self.ml = limbs(m, n)
        self.Rinv = pow(self.R, -1, m)

    def mont(self, a, b):
        return a * b * self.Rinv % self.m


def limbs(x, n):
    assert 0 <= x < (1 << (32 * n)), x
    return [(x >> (32 * i)) & MASK for i in range(n)]


def val(l):
    return sum(int(v) << (32 * i) for i, v in enumerate(l))


# ----------------------------------------------------------------------------- per-limb model
def stage_gp(stage, F, a, b):
    """(G, P) bit lists over the N limbs of one carry chain (the + m correction of a subtraction
    that did not borrow is computed as its wave-mates see it, and then discarded)"""
    N, m = F.N, F.ml
    if stage == "add":
        x, y = limbs(a, N), limbs(b, N)
        return [int(x[j] + y[j] > MASK) for j in range(N)], [int((x[j] + y[j]) & MASK == MASK) for j in range(N)]
    if stage == "reduce":
        t = limbs(a + b, N)
        return [int(t[j] < m[j]) for j in range(N)], [int(t[j] == m[j]) for j in range(N)]
    if stage == "sub":
        x, y = limbs(a, N), limbs(b, N)
        return [int(x[j] < y[j]) for j in range(N)], [int(x[j] == y[j]) for j in range(N)]
    if stage == "corr":
        d = limbs((a - b) % F.R, N)
        return [int(d[j] + m[j] > MASK) for j in range(N)], [int((d[j] + m[j]) & MASK == MASK) for j in range(N)]
    raise ValueError(stage)


def ripple(G, P):
    """carry INTO each limb, plus the carry out of the last one (N + 1 bits)"""
    c, out = 0, []
    for g, p in zip(G, P):
        out.append(c)
        c = g | (p & c)
    return out + [c]


def live_runs(G, P):
    """maximal propagate runs as (start, length, carry entering the run)"""
    cin = ripple(G, P)
    runs, j, n = [], 0, len(P)
    while j < n:
        if P[j]:
            k = j
            while k < n and P[k]:
                k += 1
            runs.append((j, k - j, cin[j]))
            j = k
        else:
            j += 1
    return runs


def wanted_runs(F, with_carry=True):
    """every (start, length) of a propagate run inside limbs 0 .. N-2 (the top limb of a sum of two
    values below m cannot be all ones); a carry can enter a run only from limb start - 1"""
    lo = 1 if with_carry else 0
    return {(j, L) for j in range(lo, F.N - 1) for L in range(1, F.N - j)}


# ----------------------------------------------------------------------------- additions
def _add_chain(F, g, j, L, carry, high):
    N, m = F.N, F.ml
    a = [g.randrange(1 << 32) for _ in range(N)]
    b = [g.randrange(1 << 32) for _ in range(N)]
    if high:  # both just below m: the sum's top limb is above m's (the reducing side)
        a[N - 1], b[N - 1] = m[N - 1] - 1 - g.randrange(16), m[N - 1] - 1 - g.randrange(16)
    else:     # the sum's top limb stays below m's (the early-out side)
        a[N - 1], b[N - 1] = g.randrange(m[N - 1] // 2), g.randrange(m[N - 1] // 2)
    for k in range(j, j + L):
        b[k] = MASK ^ a[k]
    if j > 0:
        if carry:
            a[j - 1] = g.randrange(1, 1 << 32)
            b[j - 1] = (1 << 32) - a[j - 1]
        else:
            a[j - 1], b[j - 1] = g.randrange(MASK), 0
    e = j + L
    if e < N - 1:
        a[e], b[e] = g.randrange(MASK), 0
    return val(a), val(b)


def add_cases(F, seed=0xADD):
    g = random.Random(seed ^ F.N)
    m, N = F.m, F.N
    out = []

    def put(a, b, tag):
        assert 0 <= a < m and 0 <= b < m, tag
        t = a + b
        out.append({"a": a, "b": b, "tag": tag, "cls": "early" if limbs(t, N)[N - 1] < F.ml[N - 1] else "reduce"})

    for carry in (True, False):
        for (j, L) in sorted(wanted_runs(F, carry)):
            for high in (False, True):
                put(*_add_chain(F, g, j, L, carry, high), f"chain j={j} L={L} carry={int(carry)} high={int(high)}")
    # sums at the reduction edges
    for name, s in (("m-1", m - 1), ("m", m), ("m+1", m + 1), ("2m-2", 2 * m - 2)):
        lo, hi = max(0, s - (m - 1)), min(s, m - 1)  # the range of a with a, s - a < m
        for a in sorted({lo, hi, (s + 1) // 2, lo + (hi - lo) // 3}):
            put(a, s - a, "sum " + name)
    # top limb equal to m's, the lower limbs above and below m's (rf_reduce_once's early-out edge)
    for k in range(N - 1):
        for s in (m + (1 << (32 * k)), m - (1 << (32 * k))):
            a = g.randrange(max(0, s - (m - 1)), min(s, m - 1) + 1)
            put(a, s - a, f"top-equal k={k} {'above' if s > m else 'below'}")
    # t - m with zero-limb runs of every start and length, under an incoming borrow
    for j in range(1, N):
        for L in range(1, N - j + 1):
            t = list(F.ml)
            for k in range(j - 1):
                t[k] = g.randrange(1 << 32)
            t[j - 1] = F.ml[j - 1] - 1
            e = j + L
            if e < N:
                t[e] = F.ml[e] + 1 if F.ml[e] != MASK else F.ml[e] - 1
            s = val(t)
            assert s < 2 * m - 1
            a = g.randrange(max(0, s - (m - 1)), min(s, m - 1) + 1)
            put(a, s - a, f"reduce-run j={j} L={L}")
    put(0, 0, "zero")
    put(m - 1, 0, "m-1 + 0")
    for _ in range(64):
        put(g.randrange(m), g.randrange(m), "random")
    return out


# ----------------------------------------------------------------------------- subtractions
def sub_cases(F, seed=0x5B):
    g = random.Random(seed ^ F.N)
    m, N, ml = F.m, F.N, F.ml
    out = []

    def put(a, b, tag):
        assert 0 <= a < m and 0 <= b < m, tag
        out.append({"a": a, "b": b, "tag": tag, "cls": "borrow" if a < b else "plain"})

    for v in (0, 1, m - 1, g.randrange(m)):
        put(v, v, "equal")
    for _ in range(4):  # a = b - 1: limb 0 borrows, every other limb is equal
        b = g.randrange(m) | 1
        put(b - 1, b, "b-1: borrow through every limb")
    put(m - 2, m - 1, "b-1: borrow through every limb")
    for v in (0, 1, m - 1):
        put(0, v, "0 - a")
    # zero difference limbs in runs of every start and length, under an incoming borrow
    for (j, L) in sorted(wanted_runs(F)):
        for side in (0, 1):
            b = [g.randrange(1 << 32) for _ in range(N)]
            a = [g.randrange(1 << 32) for _ in range(N)]
            lo, hi = sorted(g.sample(range(ml[N - 1]), 2))
            a[N - 1], b[N - 1] = (lo, hi) if side else (hi, lo)
            for k in range(j, j + L):
                a[k] = b[k]
            b[j - 1] |= 1
            a[j - 1] = b[j - 1] - 1
            e = j + L
            if e < N - 1:
                a[e] = b[e] ^ 1
            put(val(a), val(b), f"sub-run j={j} L={L} side={side}")
    # borrowed results whose + m correction has 0xffffffff runs with a carry entering: the result
    # r = a - b + m has zero limbs on the run and limb j-1 = m_(j-1) - 1
    for (j, L) in sorted(wanted_runs(F)):
        r = [g.randrange(1 << 32) for _ in range(N)]
        r[N - 1] = g.randrange(ml[N - 1])
        for k in range(j, j + L):
            r[k] = 0
        r[j - 1] = ml[j - 1] - 1
        e = j + L
        if e < N - 1:
            r[e] = g.randrange(1, 1 << 32)
        rv = val(r)
        assert rv < m
        b = g.randrange(m - rv, m)
        put(b + rv - m, b, f"corr-run j={j} L={L}")
    for _ in range(64):
        put(g.randrange(m), g.randrange(m), "random")
    return out


# ----------------------------------------------------------------------------- products
def operand_classes(F):
    """the multiplicative operand classes, each a list of (name, value), all canonical"""
    m, N = F.m, F.N
    cl = {
        "small": [("0", 0), ("1", 1), ("2", 2)],
        "top": [("m-1", m - 1), ("m-2", m - 2)],
        "half": [("(m-1)/2", (m - 1) // 2), ("(m+1)/2", (m + 1) // 2)],
        "mont": [("R", F.R % m), ("R2", F.R * F.R % m)],
        "pow2": [(f"2^{k}", 1 << k) for i in range(1, N) for k in (32 * i - 1, 32 * i, 32 * i + 1) if (1 << k) < m],
        "ones": [(f"ones[{j}:{j + L}]", ((1 << (32 * L)) - 1) << (32 * j)) for j in range(N - 1) for L in range(1, N - j)],
    }
    for c in cl.values():
        assert all(0 <= v < m for _, v in c)
    return cl


def mul_cases(F, seed=0x3A1):
    """every class crossed with every class: the specials pairwise in full, the two long families
    cycled against each class so that every member meets every class; plus 64 random pairs"""
    g = random.Random(seed ^ F.N)
    cl = operand_classes(F)
    out = []
    names = list(cl)
    for ca in names:
        for cb in names:
            A, B = cl[ca], cl[cb]
            if len(A) <= 3 and len(B) <= 3:
                pairs = [(x, y) for x in A for y in B]
            else:
                n = max(len(A), len(B))
                pairs = [(A[i % len(A)], B[(i + i // len(B)) % len(B)]) for i in range(n)]
                pairs += [(A[(i + i // len(A) + 1) % len(A)], B[i % len(B)]) for i in range(n)]
            for (na, a), (nb, b) in pairs:
                out.append({"a": a, "b": b, "tag": f"{na} x {nb}", "cls": ca})
    for _ in range(64):
        out.append({"a": g.randrange(F.m), "b": g.randrange(F.m), "tag": "random", "cls": "random"})
    return out


def sqr_cases(F, seed=0x591):
    g = random.Random(seed ^ F.N)
    out = [{"a": v, "tag": n, "cls": c} for c, l in operand_classes(F).items() for n, v in l]
    out += [{"a": g.randrange(F.m), "tag": "random", "cls": "random"} for _ in range(64)]
    return out


def specials(F):
    cl = operand_classes(F)
    return [v for c in ("small", "top", "half", "mont") for _, v in cl[c]]


def fq2_cases(F, seed=0xF2):
    """Fq2 operand pairs (a0, a1, b0, b1): components from the specials, every special in every
    position against every class of partner; plus 64 random"""
    g = random.Random(seed)
    S = specials(F)
    n = len(S)
    out = []
    for i in range(n):
        for k in range(n):
            a = (S[i], S[(i + k) % n])
            b = (S[(2 * i + k + 1) % n], S[(k * 3 + i) % n])
            out.append({"a": a, "b": b, "tag": "special", "cls": "c%d" % (i % 3)})
    m = F.m
    out.append({"a": (m - 1, m - 1), "b": (m - 1, m - 1), "tag": "all m-1", "cls": "c0"})
    out.append({"a": (m - 1, m - 1), "b": (m - 1, 0), "tag": "neg_in(0) partner", "cls": "c1"})
    out.append({"a": (m - 1, m - 1), "b": (0, m - 1), "tag": "neg_in(m-1) partner", "cls": "c2"})
    for _ in range(64):
        out.append({"a": (g.randrange(m), g.randrange(m)), "b": (g.randrange(m), g.randrange(m)), "tag": "random",
                    "cls": "random"})
    return out


# ----------------------------------------------------------------------------- predicates
def predicate_cases(F, seed=0x9E):
    """(a, b) for is_zero(a) and a == b: equal, zero, and values that differ in exactly one limb"""
    g = random.Random(seed ^ F.N)
    # zero beside m - 1: a row's pad lanes 12..15 load as 0, not as the words of the next operand
    out = [{"a": 0, "b": 0, "tag": "zero", "cls": "eq"}, {"a": 0, "b": F.m - 1, "tag": "zero beside m-1", "cls": "ne"}]
    v = g.randrange(F.m)
    out.append({"a": v, "b": v, "tag": "equal", "cls": "eq"})
    for j in range(F.N):
        for bit in (0, 31) if j < F.N - 1 else (0, 20):
            out.append({"a": 1 << (32 * j + bit), "b": 0, "tag": f"one limb {j}", "cls": "ne"})
            w = g.randrange(F.m >> 4)
            out.append({"a": w, "b": w ^ (1 << (32 * j + bit)), "tag": f"differ limb {j}", "cls": "ne"})
    return out


# ----------------------------------------------------------------------------- orders
def grouped(cases):
    """indices grouped by class: the rows of a wave take the same side of a wave-uniform branch"""
    order = sorted(set(c["cls"] for c in cases))
    return [i for k in order for i, c in enumerate(cases) if c["cls"] == k]


def interleaved(cases):
    """indices round-robin over the classes: every wave mixes the sides"""
    by = {}
    for i, c in enumerate(cases):
        by.setdefault(c["cls"], []).append(i)
    lists = [by[k] for k in sorted(by)]
    if len(lists) == 1:
        idx = list(lists[0])
        random.Random(7).shuffle(idx)
        return idx
    # shorter classes repeat to keep mixing; a repeated index reruns the same case
    return [l[k % len(l)] for k in range(max(len(l) for l in lists)) for l in lists]
