"""The log-derivative lookup entries (mbls_fr_lookup_multiplicities, mbls_fr_prefix_sum,
mbls_fr_logup_sum) on the GPU against the pure-Python model of tests/logup_model.py.  Every
comparison is exact equality of the element words.  The sizes are the smallest at which each
mechanism can go wrong: the scan's chunk, tile and span seams (a tile is 2048 elements), one size
past 1024 tiles per member, the join's wave and round seams, and one table past the sort's 512
one-tile workgroups."""
import ctypes
import functools
import random

import numpy as np
import pytest

import logup_model as M

pytestmark = pytest.mark.gpu

R = M.R
SEAMS = (1, 2, 2047, 2048, 2049, 3 * 2048 + 5)


def _amd():
    """the binding, with torch imported before the library is loaded"""
    import torch  # noqa: F401
    import gpu_helpers
    return gpu_helpers.amd


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _amd().lib()
    return _amd()


def words(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def ints(arr):
    data = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def small_words(v):
    """(n, 4) words of an array of integers below 2^64"""
    out = np.zeros((len(v), 4), dtype=np.uint64)
    out[:, 0] = v
    return out


def dev(a):
    return _amd().torch_u64(np.ascontiguousarray(a))


def host(t):
    return _amd().to_numpy_u64(t)


@functools.lru_cache(maxsize=None)
def small_mont():
    """Montgomery forms of 0 .. 4199, the values of the small joins"""
    return [M.mont(v) for v in range(4200)]


@functools.lru_cache(maxsize=None)
def big():
    """The shared scan reference: a column of the largest seam size mixing 0, 1, r - 1 and random
    values, and its running sum from INIT (one entry more than the column: the total)."""
    n = max(SEAMS)
    rnd = random.Random(31)
    col = [rnd.choice([0, 1, R - 1] + [rnd.randrange(R)] * 9) for _ in range(n)]
    out, total = M.prefix_sum_ref(col, INIT)
    return words(col), words(out + [total])


INIT = random.Random(7).randrange(1, R)


# ----------------------------------------------------------------------------- the additive scan
@pytest.mark.parametrize("inclusive", [False, True])
def test_prefix_sum_at_every_seam(amd, inclusive):
    col, prefix = big()
    init = words([INIT])
    for n in SEAMS:
        out, total = amd.prefix_sum(col[:n], init, inclusive, total=True)
        want = prefix[1:n + 1] if inclusive else prefix[:n]
        assert np.array_equal(out, want), n
        assert np.array_equal(total, prefix[n:n + 1]), n
        # no init is zero, no total is no second result
        plain = amd.prefix_sum(col[:n], inclusive=inclusive)
        assert ints(plain) == [(v - INIT) % R for v in ints(want)], n


def test_prefix_sum_batch_members_take_their_own_init(amd):
    col, _ = big()
    n, b = 2049, 3
    x = col[:b * n]
    rnd = random.Random(9)
    per = [rnd.randrange(R) for _ in range(b)]
    out, total = amd.prefix_sum(x, words(per), batch=b, total=True)
    for k in range(b):
        want, wt = M.prefix_sum_ref(ints(x[k * n:(k + 1) * n]), per[k])
        assert ints(out[k * n:(k + 1) * n]) == want and ints(total[k:k + 1]) == [wt], k
    assert len({tuple(r) for r in total.tolist()}) == b


def test_prefix_sum_placement_and_in_place(amd):
    col, prefix = big()
    n = 2049
    init = words([INIT])
    h_out, h_tot = amd.prefix_sum(col[:n], init, total=True)
    d_out, d_tot = amd.prefix_sum(dev(col[:n]), dev(init), out=amd.torch_u64((n, 4)), total=True)
    assert np.array_equal(h_out, prefix[:n]) and np.array_equal(h_tot, prefix[n:n + 1])
    assert np.array_equal(host(d_out), h_out) and np.array_equal(host(d_tot), h_tot)
    mixed = amd.prefix_sum(dev(col[:n]), init, True)  # device column, host init, host result
    assert np.array_equal(mixed, prefix[1:n + 1])
    t = dev(col[:n])
    assert amd.prefix_sum(t, init, out=t) is t and np.array_equal(host(t), h_out)
    h = col[:n].copy()
    amd.prefix_sum(h, init, True, out=h)
    assert np.array_equal(h, prefix[1:n + 1])


def test_prefix_sum_spans_of_several_tiles(amd):
    """2^21 + 2049 elements: past 1024 tiles, so every workgroup walks more than one.  A constant
    column: out[i] = init + i * c mod r on every row."""
    n = (1 << 21) + 2049
    assert amd.scan_geometry(n)["span"] > amd.scan_geometry(n)["tile"]
    c = random.Random(3).randrange(R)
    x = dev(np.tile(words([c]), (n, 1)))
    out, total = amd.prefix_sum(x, words([INIT]), out=amd.torch_u64((n, 4)), total=True)
    got = host(out).astype(object)
    got = got[:, 0] + (got[:, 1] << 64) + (got[:, 2] << 128) + (got[:, 3] << 192)
    want = (np.arange(n, dtype=object) * c + INIT) % R
    assert np.array_equal(got, want)
    assert ints(host(total)) == [(INIT + n * c) % R]


def test_prefix_sum_carry_extremes(amd):
    n = 3 * 2048 + 5
    wrap = np.tile(words([R - 1]), (n, 1))  # every addition wraps
    out, total = amd.prefix_sum(wrap, None, True, total=True)
    assert ints(out) == [(R - i) % R for i in range(1, n + 1)] and ints(total) == [(R - n) % R]
    out, total = amd.prefix_sum(wrap, words([R - 1]), total=True)
    assert ints(out) == [R - i for i in range(1, n + 1)] and ints(total) == [R - n - 1]
    zero = np.zeros((n, 4), dtype=np.uint64)
    out, total = amd.prefix_sum(zero, total=True)
    assert not out.any() and not total.any()
    out, total = amd.prefix_sum(zero, words([INIT]), True, total=True)
    assert np.array_equal(out, np.tile(words([INIT]), (n, 1))) and ints(total) == [INIT]


# ----------------------------------------------------------------------------- the join
def _check_join(amd, inputs, table, credit, montgomery=True, batch=1, **kw):
    """inputs, table: lists of stored integers; compares m and n_missing with the model per member"""
    m, missing = amd.lookup_multiplicities([words(c) for c in inputs], words(table), credit, montgomery, batch=batch, **kw)
    n = len(table) // batch
    got = ints(m)
    for k in range(batch):
        s = slice(k * n, (k + 1) * n)
        counts, miss = M.multiplicities_ref([c[s] for c in inputs], table[s], credit)
        assert got[s] == M.count_elements(counts, montgomery), (k, credit)
        assert missing[k] == miss, (k, credit)
        assert sum(counts) + miss == len(inputs) * n
    return got, missing


@pytest.mark.parametrize("k", [1, 3])
def test_join_on_a_shuffled_range(amd, k):
    mont = small_mont()
    for n in (1, 63, 64, 65, 2047, 2048, 2049):
        rnd = random.Random(n * 7 + k)
        table = [mont[v] for v in rnd.sample(range(n), n)]  # all rows distinct
        inputs = [[mont[rnd.randrange(n)] for _ in range(n)] for _ in range(k)]
        for credit in ("first", "last"):  # no duplicates: the two rules agree
            got, missing = _check_join(amd, inputs, table, credit)
            assert missing == [0]


@pytest.mark.parametrize("credit", ["first", "last"])
def test_join_with_every_table_value_duplicated(amd, credit):
    mont = small_mont()
    for n in (2, 64, 130, 2049):
        rnd = random.Random(n)
        vals = [mont[v] for v in range(n // 2)]
        table = vals + vals + [mont[4100]] * (n % 2)
        rnd.shuffle(table)
        inputs = [[rnd.choice(vals) for _ in range(n)] for _ in range(2)]
        got, missing = _check_join(amd, inputs, table, credit)
        assert missing == [0]
        # one credited row per value: the other holds zero
        assert sum(1 for c in got if c) <= n // 2


def test_join_of_one_repeated_value(amd):
    """every cell the same: each wave carries its count in a register across its rounds"""
    mont = small_mont()
    for n, k in ((65, 1), (2049, 3), (16 * 1024 + 70, 2)):
        table = [mont[v % 4200] for v in range(n)]
        inputs = [[mont[5 % n]] * n for _ in range(k)]
        for credit in ("first", "last"):
            got, missing = _check_join(amd, inputs, table, credit)
            assert missing == [0] and sorted(got)[-1] == M.mont(k * n) and sum(1 for c in got if c) == 1


def test_join_counts_missing_cells(amd):
    mont = small_mont()
    n, k = 2049, 3
    rnd = random.Random(12)
    table = [mont[v] for v in rnd.sample(range(n), n)]
    inputs = [[mont[rnd.randrange(n)] for _ in range(n)] for _ in range(k)]
    absent = rnd.sample(range(k * n), 37)
    for a in absent:  # values the table lacks: above it, and one the same in many cells
        inputs[a // n][a % n] = mont[n + 1 + a % 5]
    for credit in ("first", "last"):
        got, missing = _check_join(amd, inputs, table, credit)
        assert missing == [37]
    # nothing matches at all
    m, missing = amd.lookup_multiplicities([words([mont[4199]] * n)], words(table))
    assert missing == [n] and not m.any()


@pytest.mark.parametrize("montgomery", [True, False])
def test_join_of_full_width_elements(amd, montgomery):
    rnd = random.Random(77)
    n = 2049
    pool = [rnd.randrange(R) for _ in range(700)] + [0, 1, R - 1]
    table = [rnd.choice(pool) for _ in range(n)]
    inputs = [[rnd.choice(pool) for _ in range(n)] for _ in range(2)]
    for credit in ("first", "last"):
        _check_join(amd, inputs, table, credit, montgomery)


def test_join_batch_members_use_their_own_table(amd):
    mont = small_mont()
    n, b = 2049, 3
    rnd = random.Random(4)
    table, inputs = [], [[], []]
    for k in range(b):
        vals = rnd.sample(range(4000), n // (k + 1))  # member k: about k + 1 rows per value
        t = [mont[rnd.choice(vals)] for _ in range(n)]
        table += t
        for col in inputs:
            col += [rnd.choice(t) if rnd.random() < 0.9 else mont[4100 + k] for _ in range(n)]
    for credit in ("first", "last"):
        got, missing = _check_join(amd, inputs, table, credit, batch=b)
        assert all(missing)
    # device operands, device result, no count: the same words
    m, none = amd.lookup_multiplicities([dev(words(c)) for c in inputs], dev(words(table)), "last", batch=b, count=False)
    assert none is None and ints(host(m)) == got


@pytest.mark.parametrize("credit", ["first", "last"])
def test_join_past_the_sorts_one_tile_workgroups(amd, credit):
    """2^20 + 1 rows of a 16-bit range table, standard form, against numpy.bincount"""
    n = (1 << 20) + 1
    assert amd.sort_plan(n)["groups"] < -(-n // amd.sort_plan(n)["tile"])  # workgroups of several tiles
    rng = np.random.default_rng(5)
    table = np.arange(n, dtype=np.uint64) & np.uint64(0xffff)
    cells = rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
    cells[::4099] = 1 << 16  # absent
    m, missing = amd.lookup_multiplicities([dev(small_words(cells))], dev(small_words(table)), credit, False)
    absent = int((cells >> np.uint64(16)).astype(bool).sum())
    assert missing == [absent]
    counts = np.bincount(cells[cells < (1 << 16)].astype(np.int64), minlength=1 << 16).astype(np.uint64)
    want = np.zeros(n, dtype=np.uint64)
    if credit == "first":
        want[:1 << 16] = counts
    else:  # the highest row of value v: v + 15 * 2^16, and row 2^20 for v = 0
        want[15 << 16:16 << 16] = counts
        want[15 << 16], want[1 << 20] = 0, counts[0]
    assert np.array_equal(host(m), small_words(want))


# ----------------------------------------------------------------------------- terms and the sum
def _lookup(n, k, seed, zeros=False):
    """a satisfied lookup of k columns over a table of n rows (Montgomery integers), beta, and m"""
    rnd = random.Random(seed)
    pool = [M.mont(rnd.randrange(R)) for _ in range(max(1, n // 3))]
    table = [rnd.choice(pool) for _ in range(n)]
    inputs = [[rnd.choice(table) for _ in range(n)] for _ in range(k)]
    beta = M.mont(rnd.randrange(R))
    if zeros:  # a table value and an input cell whose denominator is zero
        nb, old = (R - beta) % R, table[0]
        table = [nb if t == old else t for t in table]
        inputs = [[nb if v == old else v for v in c] for c in inputs]
        inputs[-1][n // 2] = nb
        inputs[0][n - 1] = nb
    counts, missing = M.multiplicities_ref(inputs, table)
    assert missing == 0
    return inputs, table, M.count_elements(counts), beta


@pytest.mark.parametrize("k", [1, 4])
def test_logup_sum_equals_the_model(amd, k):
    for n in (1, 64, 65, 2049):
        inputs, table, m, beta = _lookup(n, k, 10 * n + k)
        rnd = random.Random(n)
        m = [M.mont(rnd.randrange(R)) if rnd.random() < 0.5 else v for v in m]  # any m, not only the right one
        want, wt = M.logup_sum_ref(inputs, table, m, beta, INIT)
        out, total = amd.logup_sum([words(c) for c in inputs], words(table), words(m), words([beta]), words([INIT]),
                                   total=True)
        assert ints(out) == want and ints(total) == [wt], n


def test_logup_sum_inverse_of_zero_is_zero(amd):
    n, k = 65, 2
    inputs, table, m, beta = _lookup(n, k, 3, zeros=True)
    nb = (R - beta) % R
    assert nb in table and inputs[0][n - 1] == nb and inputs[1][n // 2] == nb
    want, wt = M.logup_sum_ref(inputs, table, m, beta)
    out, total = amd.logup_sum([words(c) for c in inputs], words(table), words(m), words([beta]), total=True)
    assert ints(out) == want and ints(total) == [wt]
    # the rows with a zero denominator contribute the other cells' inverses only
    terms = M.terms_ref(inputs, table, m, beta)
    i = n - 1
    alone = (M.minv((inputs[1][i] + beta) % R) - M.mmul(m[i], M.minv((table[i] + beta) % R))) % R
    assert terms[i] == alone


def test_logup_sum_placement_batch_and_in_place(amd):
    n, b, k = 2049, 2, 3
    parts = [_lookup(n, k, 50 + j) for j in range(b)]
    inputs = [sum((p[0][c] for p in parts), []) for c in range(k)]
    table, m = sum((p[1] for p in parts), []), sum((p[2] for p in parts), [])
    beta = [p[3] for p in parts]
    init = [INIT, 0]
    out, total = amd.logup_sum([words(c) for c in inputs], words(table), words(m), words(beta), words(init), batch=b,
                               total=True)
    for j in range(b):
        s = slice(j * n, (j + 1) * n)
        want, wt = M.logup_sum_ref([c[s] for c in inputs], table[s], m[s], beta[j], init[j])
        assert ints(out[s]) == want and ints(total[j:j + 1]) == [wt] == [init[j]], j  # satisfied: the sum closes
    # device operands; the output takes the multiplicity column's place
    dm = dev(words(m))
    got, dt = amd.logup_sum([dev(words(c)) for c in inputs], dev(words(table)), dm, dev(words(beta)), dev(words(init)),
                            out=dm, total=True, batch=b)
    assert got is dm and np.array_equal(host(dm), out) and np.array_equal(host(dt), total)


def test_multiplicities_then_sum_closes_only_for_a_satisfied_lookup(amd):
    n, k = 2049, 2
    inputs, table, _, beta = _lookup(n, k, 99)
    cols, tab, b = [dev(words(c)) for c in inputs], dev(words(table)), words([beta])
    for credit in ("first", "last"):
        m, missing = amd.lookup_multiplicities(cols, tab, credit)
        phi, total = amd.logup_sum(cols, tab, m, b, out=amd.torch_u64((n, 4)), total=True)
        assert missing == [0] and not host(total).any() and not host(phi[:1]).any() and host(phi).any()
    bad = [list(c) for c in inputs]
    bad[1][n // 3] = next(v for v in (M.mont(x) for x in range(1, 99)) if v not in table)
    cols = [dev(words(c)) for c in bad]
    m, missing = amd.lookup_multiplicities(cols, tab)
    _, total = amd.logup_sum(cols, tab, m, b, out=amd.torch_u64((n, 4)), total=True)
    assert missing == [1] and host(total).any()


def test_no_allocation_per_call(amd):
    n, k = 3 * 2048 + 5, 2
    inputs, table, m, beta = _lookup(n, k, 123)
    hc, ht, hm, hb = [words(c) for c in inputs], words(table), words(m), words([beta])
    cols, tab, dm, db = [dev(c) for c in hc], dev(ht), dev(hm), dev(hb)
    out, tot = amd.torch_u64((n, 4)), amd.torch_u64((1, 4))

    def calls():
        amd.lookup_multiplicities(cols, tab, out=out)
        amd.lookup_multiplicities(hc, ht, "last")  # staged: the largest footprint
        amd.prefix_sum(dm, out=out, total=tot)
        amd.prefix_sum(hm, total=True)
        amd.logup_sum(cols, tab, dm, db, out=out, total=tot)
        amd.logup_sum(hc, ht, hm, hb, total=True)

    calls()
    mallocs = amd.scratch_stats()[0]
    for _ in range(10):
        calls()
    assert amd.scratch_stats()[0] == mallocs
