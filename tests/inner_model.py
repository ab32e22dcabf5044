"""Pure-Python model of the Fr inner products (csrc/inner.hip): the plain sums as the reference, and
the scheme the kernels run -- blocks of CB columns by VB vectors, consecutive tiles per workgroup,
radix-2^29 product columns of `defer` rows added into one 64-bit accumulator each before a single
Montgomery reduction by 2^261, per-workgroup partial sums folded and doubled five times --
parameterised by its geometry so that a test can run it at toy sizes.  Values are the stored words
as integers: Montgomery form, canonical."""
from collections import namedtuple

from helpers import pyref as pr

R = pr.R
ONE = pr.FR_R  # Montgomery one
RINV = pr.FR_RINV
mmul = pr.fr_mont_mul


def mont(x):
    return pr.fr_to_mont(x % R)


# ----------------------------------------------------------------------------- references
def inner_products_ref(cols, vecs):
    """out[p * len(vecs) + k] = sum_i cols[p][i] * vecs[k][i] as field elements, Montgomery form"""
    return [sum(a * b for a, b in zip(c, v)) * RINV % R for c in cols for v in vecs]


def powers_ref(base, n, init=ONE):
    """[init * base^i for i < n]: base^0 = 1 whatever the base"""
    out, run = [], init
    for _ in range(n):
        out.append(run)
        run = mmul(run, base)
    return out


def multi_eval_ref(cols, points):
    """out[p * len(points) + k] = cols[p](points[k]), coefficients lowest degree first"""
    n = len(cols[0])
    return inner_products_ref(cols, [powers_ref(z, n) for z in points])


def pow_log(n):
    """s of the two power tables: ceil(ceil(log2 n) / 2)"""
    lg = (n - 1).bit_length()
    return (lg + 1) // 2


def powers_split(base, n, init=ONE, s=None):
    """the two-table form: hi[i >> s] * lo[i & (2^s - 1)], hi[j] = init * base^(j 2^s), lo[j] = base^j,
    each table entry by square-and-multiply over the bits of its index"""
    s = pow_log(n) if s is None else s

    def by_index(x, e):
        acc = ONE
        for b in bin(e)[2:]:
            acc = mmul(acc, acc)
            if b == "1":
                acc = mmul(acc, x)
        return acc

    nlo = 1 << s
    nhi = -(-n // nlo)
    step = base
    for _ in range(s):
        step = mmul(step, step)
    lo = [by_index(base, j) for j in range(nlo)]
    hi = [mmul(by_index(step, j), init) for j in range(nhi)]
    return [mmul(hi[i >> s], lo[i & (nlo - 1)]) for i in range(n)]


# ----------------------------------------------------------------------------- radix 2^29, deferred
NL = 9
NCOL = 2 * NL - 1
MASK = (1 << 29) - 1
RL = [(R >> (29 * i)) & MASK for i in range(NL)]
DEFER = 7
# the bound stated in inner.hip: a column of one product of word operands (limbs < 2^29) is below
# 9 * 2^58, so DEFER of them, plus the carry of the normalising sweep, stay below 2^64 -- and one
# more product would not
COLUMN_BOUND = 9 * (MASK * MASK)
assert DEFER * COLUMN_BOUND + (1 << 35) < 1 << 64 <= (DEFER + 1) * COLUMN_BOUND
assert RL[0] == 1 and sum(l << (29 * i) for i, l in enumerate(RL)) == R


def unpack29(x):
    """a word value (< 2^256) as 9 limbs, the top one holding bits 232..255"""
    assert 0 <= x < 1 << 256
    return [(x >> (29 * i)) & MASK for i in range(NL - 1)] + [x >> (29 * (NL - 1))]


def mac_columns(acc, a, b):
    """acc[k] += sum_{i + j = k} a_i b_j; every accumulator is a 64-bit register"""
    for k in range(NCOL):
        acc[k] += sum(a[i] * b[k - i] for i in range(max(0, k - NL + 1), min(k, NL - 1) + 1))
        assert acc[k] < 1 << 64, "an unreduced column left 64 bits"


def reduce_columns(acc):
    """the columns of <= DEFER products of canonical operands -> T / 2^261 mod r, canonical"""
    total = sum(c << (29 * k) for k, c in enumerate(acc))
    t, carry = [], 0
    for k in range(NCOL):
        s = acc[k] + carry
        assert s < 1 << 64, "the carry sweep left 64 bits"
        t.append(s & MASK)
        carry = s >> 29
    assert carry < 1 << 20  # T < 7 r^2 < 2^513
    t.append(carry)
    col, m, out = 0, [], [0] * NL
    for k in range(NCOL):
        col += t[k] + sum(m[i] * RL[k - i] for i in range(max(0, k - NL + 1), min(k, NL)))
        assert col < 1 << 64
        if k < NL:
            m.append(-col & MASK)
            col += m[k]
            assert col & MASK == 0
        else:
            out[k - NL] = col & MASK
        col >>= 29
    out[NL - 1] = col + t[NCOL]
    v = sum(l << (29 * i) for i, l in enumerate(out))
    assert out[NL - 1] < 1 << 24 and v < 2 * R
    v = v - R if v >= R else v
    assert v == total * pow(1 << 261, -1, R) % R
    return v


# threads per workgroup, rows a thread takes from a tile (= products per reduction), columns and
# vectors per block, consecutive tiles per workgroup
Geometry = namedtuple("Geometry", "threads defer CB VB tpg")


def blocked_inner(cols, vecs, g, stats=None):
    """the two launches.  stats, a dict, receives the largest column and the most products any
    accumulator held."""
    assert g.defer <= DEFER
    n, nc, nv = len(cols[0]), len(cols), len(vecs)
    span = g.tpg * g.threads * g.defer
    groups = -(-n // span)
    peak = most = 0
    out = [None] * (nc * nv)
    for c0 in range(0, nc, g.CB):
        for v0 in range(0, nv, g.VB):
            for c in range(c0, min(c0 + g.CB, nc)):
                for v in range(v0, min(v0 + g.VB, nv)):
                    partial = []
                    for grp in range(groups):
                        end = min(n, (grp + 1) * span)
                        run = [0] * g.threads
                        for t in range(g.tpg):
                            for tid in range(g.threads):
                                acc, held = [0] * NCOL, 0
                                for j in range(g.defer):
                                    i = grp * span + (t * g.defer + j) * g.threads + tid
                                    if i < end:
                                        mac_columns(acc, unpack29(cols[c][i]), unpack29(vecs[v][i]))
                                        held += 1
                                peak, most = max(peak, max(acc)), max(most, held)
                                run[tid] = (run[tid] + reduce_columns(acc)) % R
                        partial.append(sum(run) % R)
                    out[c * nv + v] = 32 * sum(partial) % R  # S R / 32 -> S R: five doublings
    if stats is not None:
        stats.update(peak=peak, most=most)
    return out
