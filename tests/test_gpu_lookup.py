"""mbls_fr_sort and mbls_fr_lookup_permute on the GPU.  Every comparison is exact equality of words.
Small cases are held against tests/lookup_model.py in Python integers; the large ones are in standard
form, so that the expectation is numpy.lexsort over the words, computed once for the largest size and
filtered down to every prefix.  Sizes come from mbls_fr_sort_plan: the tile seams, and both sides of
the size at which a workgroup first takes a second tile (for the lookup, which sorts 2 * size elements
and scans 2 * size + 1 rank words with the same tile, that is at half those sizes)."""
import functools
import random

import numpy as np
import pytest

import lookup_model as M

pytestmark = pytest.mark.gpu

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
TOP = 0x73eda753299d7d48  # a top limb below r's: the element is canonical whatever the rest


def _amd():
    """the binding, with torch imported before the library is loaded (see test_gpu_scan.py)"""
    import torch  # noqa: F401
    import gpu_helpers
    return gpu_helpers.amd


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _amd().lib()
    return _amd()


def mont(v):
    from helpers import pyref as pr
    return pr.fr_to_mont(v % R)


def words(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def ints(arr):
    data = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def dev(a):
    return _amd().torch_u64(np.ascontiguousarray(a))


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def geometry():
    """(T, n2): elements per tile, and the first size at which a workgroup takes two tiles"""
    plan = _amd().sort_plan
    T = plan(1)["tile"]
    two = lambda n: plan(n)["groups"] * T < n
    lo, hi = 1, 1 << 26
    assert not two(lo) and two(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if two(mid) else (mid, hi)
    assert plan(hi)["groups"] < plan(lo)["groups"] and hi <= (1 << 21)
    return T, hi


def sort_sizes():
    T, n2 = geometry()
    return sorted({1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, n2 - 1, n2, n2 + 1})


def lookup_sizes():
    """the sort's seams at half the size: 2 * size elements are sorted, 2 * size + 1 words scanned"""
    T, n2 = geometry()
    h = n2 // 2  # the sort's workgroups take a second tile above h rows, the scan's from h rows on
    return sorted({1, 2, 63, 64, 65, T // 2 - 1, T // 2, T // 2 + 1, T - 1, T, T + 1, 2 * T + 3, h - 1, h, h + 1})


@functools.lru_cache(maxsize=None)
def big():
    """The shared column: n2 + 1 full-width standard-form elements drawn from a pool of a third as
    many (so duplicates abound), and `order`, its stable ascending permutation.  The sorted
    permutation of the prefix of length n is order[order < n]."""
    n = geometry()[1] + 1
    rng = np.random.default_rng(7)
    pool = rng.integers(0, 1 << 63, size=(n // 3, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(
        0, 2, size=(n // 3, 4), dtype=np.uint64)
    pool[:, 3] %= np.uint64(TOP)
    col = np.ascontiguousarray(pool[rng.integers(0, len(pool), size=n)])
    order = np.lexsort((col[:, 0], col[:, 1], col[:, 2], col[:, 3]))  # stable; the last key is the primary
    return col, order


def test_reference_prefix_filter_matches_the_model():
    col, order = big()
    n = 300
    want, perm = M.sort_ref(ints(col[:n]))
    assert order[order < n].tolist() == perm and ints(col[order[order < n]]) == want


# ----------------------------------------------------------------------------- sort
def test_sort_random_full_width_at_every_seam(amd):
    col, order = big()
    for n in sort_sizes():
        out, perm = amd.fr_sort(col[:n], mont=False, perm=True)
        want = order[order < n]
        assert np.array_equal(perm, want.astype(np.uint32)), n
        assert np.array_equal(out, col[want]), n


def test_sort_every_digit_position(amd):
    vals = [0, R - 1] + [1 << b for b in range(255)]
    random.Random(3).shuffle(vals)
    out, perm = amd.fr_sort(words(vals), mont=False, perm=True)
    assert ints(out) == sorted(vals)
    assert [vals[i] for i in perm.tolist()] == sorted(vals)
    assert (ints(out), perm.tolist()) == M.radix_sort_members(vals, g=M.LIBRARY)


def test_sort_all_equal_and_two_values(amd):
    T, _ = geometry()
    n = T + 1
    out, perm = amd.fr_sort(words([R - 2] * n), mont=False, perm=True)
    assert perm.tolist() == list(range(n)) and ints(out) == [R - 2] * n
    vals = [(i & 1) << 200 for i in range(n)]
    out, perm = amd.fr_sort(words(vals), mont=False, perm=True)
    assert perm.tolist() == list(range(0, n, 2)) + list(range(1, n, 2))
    assert ints(out) == sorted(vals)


@pytest.mark.parametrize("which", ["top_word", "low_byte"])
def test_sort_single_varying_word(amd, which):
    T, _ = geometry()
    rnd = random.Random(4)
    n = 2 * T + 3
    if which == "top_word":
        vals = [rnd.randrange(1 << 30) << 224 for _ in range(n)]
    else:
        vals = [(7 << 130) + rnd.randrange(256) for _ in range(n)]
    out, perm = amd.fr_sort(words(vals), mont=False, perm=True)
    assert (ints(out), perm.tolist()) == M.sort_ref(vals)


def test_sort_montgomery_orders_by_the_standard_value(amd):
    stored = [mont(v) for v in range(1, 65)]
    assert sorted(stored) != stored  # sorting the stored words would give another order
    order = list(range(64))
    random.Random(6).shuffle(order)
    out, perm = amd.fr_sort(words([stored[i] for i in order]), mont=True, perm=True)
    assert ints(out) == stored
    assert [order[i] for i in perm.tolist()] == list(range(64))
    # full-width Montgomery values with duplicates, against the model on the standard values
    rnd = random.Random(16)
    pool = [rnd.randrange(R) for _ in range(40)]
    vals = [rnd.choice(pool) for _ in range(131)]
    out, perm = amd.fr_sort(words([mont(v) for v in vals]), mont=True, perm=True)
    want, wperm = M.sort_ref(vals)
    assert ints(out) == [mont(v) for v in want] and perm.tolist() == wperm


def test_sort_batch_members_equal_single_sorts(amd):
    T, _ = geometry()
    col, _ = big()
    n = T + 3
    large = col[:n].copy()
    large[:, 3] = large[:, 3] % np.uint64(1 << 60) + np.uint64(1 << 62)  # canonical: below r's top limb
    small = col[n:2 * n].copy()
    small[:, 1:] = 0
    x = np.concatenate([large, small, col[2 * n:3 * n]])
    out, perm = amd.fr_sort(x, mont=False, batch=3, perm=True)
    for k in range(3):
        s = slice(k * n, (k + 1) * n)
        o1, p1 = amd.fr_sort(x[s], mont=False, perm=True)
        assert np.array_equal(out[s], o1) and np.array_equal(perm[s], p1), k
        assert np.array_equal(o1, x[s][p1]), k
    assert (ints(out[:n]), perm[:n].tolist()) == M.sort_ref(ints(large))
    # many short members: the member number takes two digit passes
    vals = [random.Random(k).randrange(4) << (32 * (k % 8)) for k in range(600)]
    out, perm = amd.fr_sort(words(vals), mont=False, batch=300, perm=True)
    assert (ints(out), perm.tolist()) == M.sort_ref(vals, 300)


def test_sort_either_output_alone_and_placement(amd):
    T, _ = geometry()
    col, order = big()
    n = 2 * T + 3
    want = order[order < n]
    only = amd.fr_sort(col[:n], mont=False)
    assert np.array_equal(only, col[want])
    none, perm = amd.fr_sort(col[:n], mont=False, out=False, perm=True)
    assert none is None and np.array_equal(perm, want.astype(np.uint32))
    assert np.array_equal(only, col[:n][perm])
    # device-resident operands equal host-resident ones
    d_out, d_perm = amd.fr_sort(dev(col[:n]), mont=False, perm=True)
    assert np.array_equal(host(d_out).view(np.uint64), only)
    assert np.array_equal(host(d_perm).view(np.uint32), perm)


# ----------------------------------------------------------------------------- lookup
def small_permute(inp, tab):
    """(A', S') of uint64 columns whose values fit one limb, vectorised"""
    a, t = np.sort(inp), np.sort(tab)
    rep = np.concatenate([[False], a[1:] == a[:-1]])
    firsts = a[~rep]
    j = np.minimum(np.searchsorted(t, firsts), len(t) - 1)
    found = t[j] == firsts
    consumed = np.zeros(len(t), dtype=bool)
    consumed[j[found]] = True
    left = t[~consumed]
    rows = np.flatnonzero(rep)
    s = a.copy()
    s[rows] = left[len(rows) - 1 - np.arange(len(rows))]
    return a, s, int((~found).sum())


def limb0(v):
    out = np.zeros((len(v), 4), dtype=np.uint64)
    out[:, 0] = v
    return out


@functools.lru_cache(maxsize=None)
def range_columns():
    """a 16-bit range table padded with zeros and random inputs, at the largest lookup size"""
    n = lookup_sizes()[-1]
    rng = np.random.default_rng(21)
    return rng.integers(0, 1 << 16, size=n, dtype=np.uint64), np.arange(n, dtype=np.uint64) * (np.arange(n) < (1 << 16))


def test_small_permute_is_the_model():
    rnd = random.Random(2)
    for _ in range(300):
        n = rnd.randrange(1, 12)
        inp = [rnd.randrange(6) for _ in range(n)]
        tab = [rnd.randrange(7) for _ in range(n)]
        a, s, miss = small_permute(np.array(inp, dtype=np.uint64), np.array(tab, dtype=np.uint64))
        assert (a.tolist(), s.tolist(), miss) == M.permute_sequential(inp, tab)


def test_lookup_range_table_at_every_seam(amd):
    inp, tab = range_columns()
    for n in lookup_sizes():
        k = min(16, n.bit_length() - 1)  # the table 0 .. 2^k - 1 fits the n rows
        i_n, t_n = inp[:n] % np.uint64(1 << k), tab[:n] * (np.arange(n) < (1 << k))
        a, s, miss = small_permute(i_n, t_n)
        assert miss == 0
        pin, ptab, cnt = amd.lookup_permute(limb0(i_n), limb0(t_n), mont=False)
        assert cnt == [0], n
        assert np.array_equal(pin, limb0(a)), n
        assert np.array_equal(ptab, limb0(s)), n


def test_lookup_permutation_of_the_table(amd):
    """a table of distinct full-width values: no row is repeated, so S' == A' == the sorted table"""
    col, _ = big()
    for n in (lookup_sizes()[-1], 2 * geometry()[0] + 3):
        table = col[:n].copy()
        table[:, 0] = np.arange(n, dtype=np.uint64)  # distinct, whatever the upper limbs repeat
        inp = np.ascontiguousarray(table[np.random.default_rng(n).permutation(n)])
        pin, ptab, cnt = amd.lookup_permute(inp, table, mont=False)
        want = table[np.lexsort((table[:, 0], table[:, 1], table[:, 2], table[:, 3]))]
        assert cnt == [0] and np.array_equal(pin, want) and np.array_equal(ptab, want), n


def _against_model(amd, inp, tab, *, as_mont):
    enc = mont if as_mont else (lambda v: v)
    pin, ptab, cnt = amd.lookup_permute(words([enc(v) for v in inp]), words([enc(v) for v in tab]), mont=as_mont)
    a, s, miss = M.permute_sequential(inp, tab)
    assert ints(pin) == [enc(v) for v in a] and ints(ptab) == [enc(v) for v in s] and cnt == [miss]
    return miss


@pytest.mark.parametrize("as_mont", [True, False])
def test_lookup_small_cases_against_the_model(amd, as_mont):
    rnd = random.Random(12)
    tab = [rnd.randrange(R) for _ in range(70)]
    # a single input value
    assert _against_model(amd, [tab[9]] * 70, tab, as_mont=as_mont) == 0
    # a table value duplicated and used by a repeated input
    dup = tab[:60] + [tab[5]] * 10
    assert _against_model(amd, [tab[5]] * 4 + [rnd.choice(tab[:60]) for _ in range(66)], dup, as_mont=as_mont) == 0
    # heavy duplicates on both sides
    assert _against_model(amd, [rnd.choice(tab[:3]) for _ in range(70)], tab[:3] * 23 + [tab[0]], as_mont=as_mont) == 0
    # one absent value, once and in two rows: it counts once
    absent = R - 1
    assert _against_model(amd, [rnd.choice(tab) for _ in range(69)] + [absent], tab, as_mont=as_mont) == 1
    assert _against_model(amd, [rnd.choice(tab) for _ in range(68)] + [absent] * 2, tab, as_mont=as_mont) == 1
    assert _against_model(amd, [3, 9, 9, 1, 3, 9, 2, 2], [1, 2, 3, 4, 5, 6, 7, 8], as_mont=as_mont) == 1
    assert _against_model(amd, [4], [5], as_mont=as_mont) == 1
    assert _against_model(amd, [4], [4], as_mont=as_mont) == 0


def test_lookup_batch_of_three_with_different_tables(amd):
    T, _ = geometry()
    n = T // 2 + 5
    rnd = random.Random(13)
    tabs = [[rnd.randrange(R) for _ in range(n)], list(range(n)), [rnd.randrange(50) << 100 for _ in range(n)]]
    inps = [[rnd.choice(t) for _ in range(n)] for t in tabs]
    inps[2][3] = 1 << 250  # member 2 lacks one value
    pin, ptab, cnt = amd.lookup_permute(words(sum(inps, [])), words(sum(tabs, [])), mont=False, batch=3)
    assert cnt == [0, 0, 1]
    for k in range(3):
        a, s, _ = M.permute_sequential(inps[k], tabs[k])
        assert ints(pin[k * n:(k + 1) * n]) == a and ints(ptab[k * n:(k + 1) * n]) == s, k


def test_lookup_placement_and_no_allocation_per_call(amd):
    T, _ = geometry()
    inp, tab = range_columns()
    n = 2 * T + 3
    i_n, t_n = limb0(inp[:n] % np.uint64(1 << 11)), limb0(tab[:n] * (np.arange(n) < (1 << 11)))
    h_in, h_tab, h_cnt = amd.lookup_permute(i_n, t_n, mont=False)
    di, dt = dev(i_n), dev(t_n)
    outs = (amd.torch_u64((n, 4)), amd.torch_u64((n, 4)))
    d_in, d_tab, d_cnt = amd.lookup_permute(di, dt, mont=False, out=outs)
    assert d_cnt == h_cnt == [0]
    assert np.array_equal(host(d_in).view(np.uint64), h_in) and np.array_equal(host(d_tab).view(np.uint64), h_tab)
    sorted_out = amd.torch_u64((n, 4))

    def calls():
        amd.lookup_permute(di, dt, mont=False, out=outs)
        amd.lookup_permute(i_n, t_n, mont=False)  # staged: the largest footprint
        amd.fr_sort(di, mont=False, out=sorted_out)
        amd.fr_sort(i_n, mont=False, perm=True)

    calls()
    mallocs = amd.scratch_stats()[0]
    for _ in range(5):
        calls()
    assert amd.scratch_stats()[0] == mallocs
