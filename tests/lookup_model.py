"""Pure-Python model of the Fr sort and the lookup argument's permuted pair (csrc/sort.hip), in Python
integers: the sequential CPU algorithm (permute_expression_pair: sort, ordered map of counts, pop
from the back), the parallel formulation the kernels run (first / repeated rows, consumed table
entries, two rank scans, leftovers taken from the back), and the radix scheme at a geometry the
caller chooses -- word planes, the uniform-word flags, the word gather, four stable 8-bit passes of
histogram / offsets / scatter per word with the scatter's wave and round structure, and the passes
over the member number that bring a batch's members back together.  Values are standard-form
integers: the keys the library sorts by."""
from collections import namedtuple

BITS = 8
DIGITS = 1 << BITS
KEY_WORDS = 8
WORD_PASSES = 32 // BITS

Geometry = namedtuple("Geometry", "wave waves rounds max_groups")
# the library's geometry (mbls_fr_sort_plan: tile = wave * waves * rounds) and a toy one
LIBRARY = Geometry(wave=64, waves=4, rounds=8, max_groups=512)
TOY = Geometry(wave=4, waves=2, rounds=2, max_groups=3)


# ----------------------------------------------------------------------------- sequential reference
def sort_ref(vals, batch=1):
    """(sorted, perm) per member: ascending by value, ties in ascending original index"""
    n = len(vals) // batch
    out, perm = [], []
    for k in range(batch):
        order = sorted(range(n), key=lambda i: vals[k * n + i])  # sorted() is stable
        perm += order
        out += [vals[k * n + i] for i in order]
    return out, perm


def permute_sequential(inp, tab):
    """(A', S', n_missing) of one member as the CPU prover computes them: the input sorted; an
    ordered map value -> count of the table; every first occurrence of an input value takes one
    instance out of the map; the leftovers, walked in ascending order, each go to the repeated row
    popped from the back of the list.  Where the CPU stops with ConstraintSystemFailure (a value the
    table lacks) the model counts it and goes on: the walk ends when the repeated rows run out."""
    a = sorted(inp)
    counts = {}
    for v in tab:
        counts[v] = counts.get(v, 0) + 1
    s = [None] * len(a)
    repeated, missing = [], 0
    for row, v in enumerate(a):
        if row == 0 or v != a[row - 1]:
            s[row] = v
            if v in counts:
                assert counts[v] > 0
                counts[v] -= 1
            else:
                missing += 1
        else:
            repeated.append(row)
    for v in sorted(counts):
        for _ in range(counts[v]):
            if repeated:
                s[repeated.pop()] = v
    assert not repeated
    return a, s, missing


# ----------------------------------------------------------------------------- parallel formulation
def exclusive_scan(flags):
    out, run = [], 0
    for f in flags:
        out.append(run)
        run += f
    return out + [run]  # one more entry: the total


def lower_bound(t, v):
    """the first index of sorted t whose entry is not below v, by bounded halving"""
    lo, hi = 0, len(t)
    for _ in range(27):
        if lo >= hi:
            break
        mid = lo + (hi - lo) // 2
        if t[mid] < v:
            lo = mid + 1
        else:
            hi = mid
    return lo


def permute_parallel(inp, tab):
    """(A', S', n_missing) of one member, every step a map over rows or a scan"""
    n = len(inp)
    a, t = sorted(inp), sorted(tab)
    repeated = [int(i != 0 and a[i] == a[i - 1]) for i in range(n)]
    consumed, missing = [0] * n, 0
    for i in range(n):
        if not repeated[i]:
            j = lower_bound(t, a[i])
            if j < n and t[j] == a[i]:
                assert not consumed[j]  # distinct values hit distinct rows
                consumed[j] = 1
            else:
                missing += 1
    rs, cs = exclusive_scan(repeated), exclusive_scan(consumed)
    m = rs[n]
    left = [None] * n
    for j in range(n):
        if not consumed[j]:
            left[j - cs[j]] = j
    s = [a[i] if not repeated[i] else t[left[m - 1 - rs[i]]] for i in range(n)]
    return a, s, missing


# ----------------------------------------------------------------------------- the radix scheme
def sort_geom(n, g):
    """(span, groups): elements per workgroup (a whole number of tiles) and workgroups per pass"""
    tile = g.wave * g.waves * g.rounds
    tiles = -(-n // tile)
    per = max(1, -(-tiles // g.max_groups))
    span = per * tile
    return span, max(1, -(-n // span))


def member_passes(members):
    p, top = 0, members - 1
    while top:
        p, top = p + 1, top >> BITS
    return p


def digit_pass(word, idx, shift, g, stats):
    """one stable pass over the (word, index) pairs: per-workgroup histograms, the offsets table,
    the scatter in rounds of one element per thread, ranked by wave then lane"""
    n = len(word)
    span, groups = sort_geom(n, g)
    threads = g.wave * g.waves
    digit = lambda w: (w >> shift) & (DIGITS - 1)
    hist = [[0] * groups for _ in range(DIGITS)]
    for grp in range(groups):
        for i in range(grp * span, min(n, (grp + 1) * span)):
            hist[digit(word[i])][grp] += 1
    tot = [sum(row) for row in hist]
    offsets, base = [[0] * groups for _ in range(DIGITS)], 0
    for d in range(DIGITS):
        run = base
        for grp in range(groups):
            offsets[d][grp] = run
            run += hist[d][grp]
        base += tot[d]
    out_w, out_i = [None] * n, [None] * n
    for grp in range(groups):
        start, end = grp * span, min(n, (grp + 1) * span)
        run = [offsets[d][grp] for d in range(DIGITS)]
        for b in range(start, end, threads):
            wc = [[0] * DIGITS for _ in range(g.waves)]
            rank = {}
            for t in range(threads):
                if b + t < end:
                    d, wave = digit(word[b + t]), t // g.wave
                    rank[t] = wc[wave][d]  # the lanes below with the same digit
                    wc[wave][d] += 1
            for t, r in rank.items():
                d, wave = digit(word[b + t]), t // g.wave
                pos = run[d] + sum(wc[j][d] for j in range(wave)) + r
                assert out_w[pos] is None
                out_w[pos], out_i[pos] = word[b + t], idx[b + t]
            for d in range(DIGITS):
                run[d] += sum(wc[j][d] for j in range(g.waves))
    stats["passes"] += 1
    return out_w, out_i


def radix_sort(vals, batch=1, g=TOY, skip=True, stats=None):
    """the permutation (positions in the whole array, members together) the library's scheme gives"""
    stats = stats if stats is not None else {}
    stats.setdefault("passes", 0)
    stats.setdefault("skipped_words", 0)
    n = len(vals)
    size = n // batch
    planes = [[(v >> (32 * w)) & 0xFFFFFFFF for v in vals] for w in range(KEY_WORDS)]
    varies = [any(x != p[0] for x in p) for p in planes]
    idx = list(range(n))
    for w in range(KEY_WORDS):
        if skip and not varies[w]:
            stats["skipped_words"] += 1
            continue
        word = [planes[w][i] for i in idx]
        for p in range(WORD_PASSES):
            word, idx = digit_pass(word, idx, p * BITS, g, stats)
    if member_passes(batch):
        word = [i // size for i in idx]
        for p in range(member_passes(batch)):
            word, idx = digit_pass(word, idx, p * BITS, g, stats)
    return idx


def radix_sort_members(vals, batch=1, **kw):
    """(sorted, perm) in mbls_fr_sort's terms: per member, perm the index within the member"""
    size = len(vals) // batch
    idx = radix_sort(vals, batch, **kw)
    assert all(g // size == i // size for i, g in enumerate(idx)), "a member's rows hold its own elements"
    return [vals[g] for g in idx], [g % size for g in idx]
