"""Pure-Python model of the Fr scans (csrc/scan.hip): the sequential recurrences as the reference, and
the tiled scheme the kernels run -- per-thread chunks, Kogge-Stone across a wave with one uniform
multiplier per distance, the waves' aggregates in order, the span aggregates scanned by one
workgroup, the rescan from the carry-in -- parameterised by its geometry so that a test can run it
at toy sizes.  Values are Montgomery-form integers, as the library's elements are."""
from collections import namedtuple

from helpers import pyref as pr

R = pr.R
ONE = pr.FR_R  # Montgomery one
mmul = pr.fr_mont_mul


def mont(x):
    return pr.fr_to_mont(x % R)


def minv(x):
    """Montgomery inverse with 1 / 0 = 0 (batch_inv's rule)"""
    return 0 if x == 0 else mont(pow(pr.fr_from_mont(x), -1, R))


def mpow(x, e):
    acc = ONE
    for b in bin(e)[2:]:
        acc = mmul(acc, acc)
        if b == "1":
            acc = mmul(acc, x)
    return acc


# ----------------------------------------------------------------------------- sequential reference
def prefix_product_ref(num, den=None, init=ONE, inclusive=False):
    """(out, total): out[i] = init * prod_{j < i} num[j] / den[j] (inclusive: j <= i), 1 / 0 = 0"""
    # a Montgomery product is a plain product by x * R^-1: one modular product per element
    rinv = pr.FR_RINV
    fac = [x * rinv % R for x in num] if den is None else [x * minv(d) % R * rinv * rinv % R for x, d in zip(num, den)]
    out, run = [], init
    for f in fac:
        if not inclusive:
            out.append(run)
        run = run * f % R
        if inclusive:
            out.append(run)
    return out, run


def divide_ref(a, z):
    """(q, p(z)) with p = q * (X - z) + p(z): q[i-1] = a[i] + z * q[i], q[n-1] = 0"""
    zc = z * pr.FR_RINV % R
    q, run = [0] * len(a), 0
    for i in range(len(a) - 1, -1, -1):
        q[i] = run
        run = (a[i] + zc * run) % R
    return q, run


# ----------------------------------------------------------------------------- the tiled scheme
# K elements per thread, `wave` lanes (a power of two), `waves` waves per workgroup, tpg tiles per
# workgroup span, agg_k span aggregates per thread in the second launch
Geometry = namedtuple("Geometry", "K wave waves tpg agg_k")
Op = namedtuple("Op", "identity step rev")
MUL = Op(ONE, lambda run, x, m: mmul(run, x), False)
HORNER = Op(0, lambda run, x, m: (x + mmul(m, run)) % R, True)


def tile_elems(g):
    return g.K * g.wave * g.waves


def _chunks(op, src, base, size, kk, threads):
    return [[src[base + t * kk + k] if base + t * kk + k < size else op.identity for k in range(kk)]
            for t in range(threads)]


def _tile_scan(op, x, unit, run, g):
    """x[t] = thread t's chunk.  Returns (the value entering each thread's chunk, the value leaving
    the tile) for the value `run` entering the tile."""
    kk, threads = len(x[0]), g.wave * g.waves
    chunk = mpow(unit, kk)
    rank = (lambda t: g.wave - 1 - t % g.wave) if op.rev else (lambda t: t % g.wave)
    prev = (lambda t, d: t + d) if op.rev else (lambda t, d: t - d)
    v = []
    for t in range(threads):
        xs = x[t][::-1] if op.rev else x[t]
        a = xs[0]
        for e in xs[1:]:
            a = op.step(a, e, unit)
        v.append(a)
    m, d = chunk, 1
    while d < g.wave:  # Kogge-Stone, one multiplier for every lane of a step
        v = [op.step(v[prev(t, d)] if rank(t) >= d else op.identity, v[t], m) for t in range(threads)]
        m, d = mmul(m, m), 2 * d
    before = [v[prev(t, 1)] if rank(t) >= 1 else op.identity for t in range(threads)]
    agg = [v[w * g.wave + (0 if op.rev else g.wave - 1)] for w in range(g.waves)]
    acc, wave_in = run, [None] * g.waves
    for j in range(g.waves):
        w = g.waves - 1 - j if op.rev else j
        wave_in[w] = acc
        acc = op.step(acc, agg[w], m)  # m = chunk^wave
    return [op.step(wave_in[t // g.wave], before[t], mpow(chunk, rank(t))) for t in range(threads)], acc


def tiled_scan(op, xs, g, unit=ONE, init=None, inclusive=False):
    """the three launches: (out, total)"""
    n, tile, threads = len(xs), tile_elems(g), g.wave * g.waves
    span = g.tpg * tile
    groups = -(-n // span)
    assert 1 <= groups <= g.agg_k * threads
    order = (lambda k: reversed(range(k))) if op.rev else range

    def span_tiles(grp):
        nt = min(g.tpg, -(-(n - grp * span) // tile))
        return [grp * span + t * tile for t in order(nt)]

    agg = []
    for grp in range(groups):  # launch 1
        run = op.identity
        for base in span_tiles(grp):
            _, run = _tile_scan(op, _chunks(op, xs, base, n, g.K, threads), unit, run, g)
        agg.append(run)
    unit2 = mpow(unit, span)  # launch 2: one element is a whole span
    x = _chunks(op, agg, 0, groups, g.agg_k, threads)
    enter, total = _tile_scan(op, x, unit2, op.identity if init is None else init, g)
    carry = [None] * groups
    for t in range(threads):
        cur = enter[t]
        for k in order(g.agg_k):
            if t * g.agg_k + k < groups:
                carry[t * g.agg_k + k] = cur
            cur = op.step(cur, x[t][k], unit2)
    out = [None] * n
    for grp in range(groups):  # launch 3
        run = carry[grp]
        for base in span_tiles(grp):
            x = _chunks(op, xs, base, n, g.K, threads)
            enter, run = _tile_scan(op, x, unit, run, g)
            for t in range(threads):
                cur = enter[t]
                for k in order(g.K):
                    i = base + t * g.K + k
                    nxt = op.step(cur, x[t][k], unit)
                    if i < n:
                        out[i] = nxt if inclusive else cur
                    cur = nxt
    return out, total
