"""The model of tests/lookup_model.py against itself, on the CPU, without the library: the parallel
formulation of the permuted pair against the sequential CPU algorithm, and the radix scheme at toy
geometry against sorted() with stable ties."""
import random

import pytest

import lookup_model as M

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def _cases():
    rnd = random.Random(5)
    out = {}
    tab = [rnd.randrange(R) for _ in range(40)]
    out["random"] = ([rnd.choice(tab) for _ in range(40)], tab)
    out["heavy_duplicates"] = ([rnd.choice(tab[:3]) for _ in range(40)], tab[:3] * 13 + [tab[0]])
    out["table_padded"] = ([rnd.randrange(16) for _ in range(40)], list(range(16)) + [0] * 24)
    perm = tab[:]
    rnd.shuffle(perm)
    out["no_repeats"] = (perm, tab)
    out["one_value"] = ([tab[7]] * 40, tab)
    out["one_value_table_too"] = ([5] * 9, [5] * 9)
    out["missing_one"] = ([rnd.choice(tab[:20]) for _ in range(39)] + [R - 1], tab[:20] * 2)
    out["missing_repeated"] = ([3, 9, 9, 1, 3, 9, 2, 2], [1, 2, 3, 4, 5, 6, 7, 8])
    out["single_row"] = ([4], [4])
    out["single_row_missing"] = ([4], [5])
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_parallel_formulation_is_the_sequential_algorithm(name):
    inp, tab = CASES[name]
    want = M.permute_sequential(inp, tab)
    assert M.permute_parallel(inp, tab) == want
    a, s, missing = want
    assert a == sorted(inp) and None not in s
    assert missing == len(set(inp) - set(tab))
    if not missing:  # the lookup argument's own conditions
        assert sorted(s) == sorted(tab)
        assert all(a[i] == s[i] or a[i] == a[i - 1] for i in range(len(a)))


def test_parallel_formulation_on_random_small_cases():
    rnd = random.Random(1)
    for _ in range(20000):
        n = rnd.randrange(1, 9)
        top = rnd.randrange(1, 7)
        inp = [rnd.randrange(top) for _ in range(n)]
        tab = [rnd.randrange(top + rnd.randrange(2)) for _ in range(n)]
        assert M.permute_parallel(inp, tab) == M.permute_sequential(inp, tab), (inp, tab)


def test_missing_values_fill_from_the_back():
    """two rows of one absent value count once; the repeated rows take the smallest leftovers, the
    last repeated row the smallest of all"""
    a, s, missing = M.permute_sequential([3, 9, 9, 1, 3, 9, 2, 2], [1, 2, 3, 4, 5, 6, 7, 8])
    assert a == [1, 2, 2, 3, 3, 9, 9, 9] and missing == 1
    assert s == [1, 2, 7, 3, 6, 9, 5, 4]


def _radix_columns():
    rnd = random.Random(8)
    tile = M.TOY.wave * M.TOY.waves * M.TOY.rounds
    span_seam = tile * M.TOY.max_groups  # above it a workgroup takes two tiles
    cols = {}
    for n in (1, 2, M.TOY.wave + 1, tile - 1, tile, tile + 1, 2 * tile + 3, span_seam, span_seam + 1, 2 * span_seam + 5):
        pool = [rnd.randrange(R) for _ in range(max(1, n // 2))]
        cols[f"random_{n}"] = ([rnd.choice(pool) for _ in range(n)], 1)
    cols["digit_positions"] = (rnd.sample([0, R - 1] + [1 << b for b in range(255)], 257), 1)
    cols["all_equal"] = ([R - 2] * (tile + 1), 1)
    cols["two_values"] = ([(i & 1) << 200 for i in range(2 * tile + 1)], 1)
    cols["top_word_only"] = ([rnd.randrange(1 << 30) << 224 for _ in range(3 * tile)], 1)
    cols["low_byte_only"] = ([(7 << 130) + rnd.randrange(256) for _ in range(3 * tile)], 1)
    big = [rnd.randrange(R // 2, R) for _ in range(tile + 3)]
    small = [rnd.randrange(1 << 16) for _ in range(tile + 3)]
    cols["batch_3"] = (big + small + [rnd.choice(big + small) for _ in range(tile + 3)], 3)
    cols["batch_300_short_members"] = ([rnd.randrange(4) << (32 * rnd.randrange(8)) for _ in range(600)], 300)
    return cols


RADIX = _radix_columns()


@pytest.mark.parametrize("name", sorted(RADIX))
@pytest.mark.parametrize("skip", [True, False])
def test_radix_scheme_is_a_stable_sort(name, skip):
    vals, batch = RADIX[name]
    assert M.radix_sort_members(vals, batch, skip=skip) == M.sort_ref(vals, batch)


def test_uniform_words_are_skipped_and_change_nothing():
    vals, _ = RADIX["low_byte_only"]
    with_skip, without = {}, {}
    a = M.radix_sort(vals, skip=True, stats=with_skip)
    b = M.radix_sort(vals, skip=False, stats=without)
    assert a == b
    assert with_skip == {"passes": 4, "skipped_words": 7} and without == {"passes": 32, "skipped_words": 0}
    batch = {}
    M.radix_sort(RADIX["batch_300_short_members"][0], 300, skip=False, stats=batch)
    assert batch["passes"] == 32 + 2  # the member number of 300 members has two digits


def test_geometry_covers_every_size():
    for g in (M.TOY, M.LIBRARY):
        tile = g.wave * g.waves * g.rounds
        for n in (1, tile, tile + 1, tile * g.max_groups, tile * g.max_groups + 1, 5 * tile * g.max_groups + 7):
            span, groups = M.sort_geom(n, g)
            assert span % tile == 0 and groups <= g.max_groups
            assert (groups - 1) * span < n <= groups * span
