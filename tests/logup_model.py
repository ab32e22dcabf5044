"""Pure-Python model of the log-derivative lookup entries (csrc/logup.hip): the multiplicity join as
a dictionary walk, the running sum as a loop, the terms with 1 / 0 = 0, and the additive operator of
the scan skeleton for tests/scan_model.py's tiled scheme.  Field values are Montgomery-form
integers, as the library's elements are; the join compares the stored integers, which is equality of
the canonical elements in either form."""
import scan_model as S

R = S.R
ONE = S.ONE
mont = S.mont
mmul = S.mmul
minv = S.minv

# the scan skeleton's third operator: one modular addition, no multiplier
ADD = S.Op(0, lambda run, x, m: (run + x) % R, False)


def multiplicities_ref(inputs, table, credit="first"):
    """(counts, n_missing) of one member: counts[j] = the cells of `inputs` (a list of columns) equal
    to table[j] when j is the credited row of its value -- the lowest row holding it, or the highest
    for credit == "last" -- else 0; n_missing = the cells whose value the table lacks."""
    row = {}
    for j, v in enumerate(table):
        if credit == "last" or v not in row:
            row[v] = j
    counts, missing = [0] * len(table), 0
    for col in inputs:
        for v in col:
            if v in row:
                counts[row[v]] += 1
            else:
                missing += 1
    return counts, missing


def multiplicities_brute(inputs, table, credit="first"):
    """the header's formula, read literally: quadratic, for small cases"""
    n = len(table)
    counts = []
    for j in range(n):
        rows = [i for i in range(n) if table[i] == table[j]]
        credited = rows[-1] if credit == "last" else rows[0]
        counts.append(sum(1 for col in inputs for v in col if v == table[j]) if credited == j else 0)
    missing = sum(1 for col in inputs for v in col if all(v != t for t in table))
    return counts, missing


def count_elements(counts, montgomery=True):
    return [mont(c) if montgomery else c for c in counts]


def prefix_sum_ref(col, init=0, inclusive=False):
    """(out, total): out[i] = init + sum_{j < i} col[j] (inclusive: j <= i)"""
    out, run = [], init
    for x in col:
        if not inclusive:
            out.append(run)
        run = (run + x) % R
        if inclusive:
            out.append(run)
    return out, run


def terms_ref(inputs, table, m, beta):
    """term[i] = sum_c 1 / (inputs[c][i] + beta) - m[i] / (table[i] + beta), 1 / 0 = 0; Montgomery"""
    out = []
    for i in range(len(table)):
        t = sum(minv((col[i] + beta) % R) for col in inputs)
        t -= mmul(m[i], minv((table[i] + beta) % R))
        out.append(t % R)
    return out


def logup_sum_ref(inputs, table, m, beta, init=0):
    """(phi[0 .. n), phi[n])"""
    return prefix_sum_ref(terms_ref(inputs, table, m, beta), init)
