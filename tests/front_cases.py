"""The inputs that put the MSM front on each side of its branches, at the smallest size that flips
the branch (tests/test_front_model.py on the CPU, tests/test_gpu_front.py on the device).

A case pins the plan fields it was designed for (so coverage cannot drift when auto_c or shift_plan
change) and its cell of front_model.census.  Sizes are written in terms of the constants
front_model parses from the sources.  Most cases live on the unsplit G1 plan (bitsize = 128,
c = 16), where the scalar d 2^(16 w) puts its point into bucket d - 1 of window w and nowhere else
and (2^16 - d) 2^(16 w) gives the digit -d with a carry; `glv` mirrors run the same scalars
through the G1 GLV plan (below lambda / 2 they are their own first half) and `psi` through G2's."""
from dataclasses import dataclass, field
from typing import Callable

import front_model as fm
from helpers import pyref as pr
import helpers as H

T, L, SM, HS = fm.DT_TILE, fm.CHUNK, fm.SMALL_MAX, fm.HEAVY_SLICE
UNSPLIT = dict(c=16, bitsize=128)
UNSPLIT_PLAN = dict(c=16, W=9, Wg=9, F=1, sF=0, split=1, prepared=0, bstride=1, partition_sort=1,
                    fused_chunk_counts=1, chunk=L)
UNSPLIT13 = dict(c=13, bitsize=128)  # FB = 4: k_chunk_counts, not the fused form
UNSPLIT13_PLAN = dict(c=13, W=10, Wg=10, F=1, sF=0, split=1, partition_sort=1, fused_chunk_counts=0, chunk=L)
GLV = dict(c=16)
GLV_PLAN = dict(c=16, W=8, Wg=8, F=1, sF=0, split=2, prepared=0, bstride=1, partition_sort=1, fused_chunk_counts=1,
                chunk=L)
PSI = dict(c=16)
PSI_PLAN = dict(c=16, W=4, Wg=4, F=1, sF=0, split=4, prepared=0, bstride=1, partition_sort=1, fused_chunk_counts=1,
                chunk=L)


@dataclass
class Case:
    name: str
    group: str
    cfg: dict                      # c, bitsize, precompute_factor
    scalars: Callable[[], list]    # standard-form integers
    plan: dict                     # the plan fields the case was designed for
    cell: Callable[[dict], bool]   # its census cell
    bases: str = "none"            # "none": null bases; "plain": n points; "table": n F table entries
    mont: bool = False             # hand the scalars over in Montgomery form
    n: int = field(default=0)


def dig(d, w, c=16):
    """the scalar whose only digits are d in window w (and, for d < 0, the carry 1 in window w + 1)"""
    return (d if d > 0 else (1 << c) + d) << (c * w)


def part_digits(part, k, c=16, spread=None):
    """k digits of one part (128 fine buckets at c = 16), over `spread` of its fine buckets"""
    fbn = 1 << fm.sort_sizes(dict(B=1 << (c - 1), pts=1, split=1, F=1))["FB"]
    spread = fbn if spread is None else spread
    return [part * fbn + 1 + i % spread for i in range(k)]


def layout(specs, c=16, w=0):
    """scalars filling consecutive buckets of window w: specs = [(start mod L or None, entries)];
    pad buckets are put in front of a bucket to give it its start"""
    out, off, d = [], 0, 1
    for start, count in specs:
        if start is not None and off % L != start:
            pad = (start - off) % L
            out += [dig(d, w, c)] * pad
            off, d = off + pad, d + 1
        out += [dig(d, w, c)] * count
        off, d = off + count, d + 1
    return out


# the chunk tables' cells: (bucket start mod L, chunk count), each count at an aligned start and at L - 1
CHUNK_SPECS = [(0, 1), (L - 1, 1), (0, 2), (L - 1, 2), (0, SM * L), (L - 1, (SM - 1) * L + 1), (0, SM * L + 1),
               (L - 1, (SM - 1) * L + 2), (0, (SM - 1) * L + 2), (0, 0), (L - 1, 0), (0, 32 * L), (0, 32 * L + 1),
               (L - 1, 31 * L + 1), (L - 1, 31 * L + 2)]
CHUNK_CELLS = {(0, 0), (L - 1, 0), (0, 1), (L - 1, 1), (L - 1, 2), (0, SM), (L - 1, SM), (0, SM + 1), (L - 1, SM + 1),
               (0, 32), (0, 33), (L - 1, 32), (L - 1, 33)}


def chunk_cell(z):
    return (CHUNK_CELLS <= z["chunk_cells"] and z["end_on_chunk"] and z["owner_queued"] == 2 and z["owner_direct"] > 0
            and z["heavy_plan"] == "planned" and z["max_slices"] == 1)


def many_heavy(c, windows):
    """HEAVY_LDS + 1 or more buckets above SMALL_MAX chunks, one per part so that no part is heavy:
    every point sits in bucket d - 1 of `windows` windows"""
    fbn = 1 << fm.sort_sizes(dict(B=1 << (c - 1), pts=1, split=1, F=1))["FB"]
    per = -(-(fm.HEAVY_LDS + 1) // windows)
    rep = sum(1 << (c * w) for w in range(windows))
    return [(1 + fbn * k) * rep for k in range(per) for _ in range(SM * L + 1)]


def rand(seed, n, bits):
    g = pr.rng(seed)
    return [g.getrandbits(bits) for _ in range(n)]


def full_width(seed, n, edges):
    """random scalars, the split's boundary scalars, and scalars at and above r"""
    g = pr.rng(seed)
    return [g.randrange(pr.R) for _ in range(n)] + list(edges) + [pr.R - 1, pr.R, pr.R + 5, (1 << 256) - 1]


def _heavy1(z, helpers, segments, empty, fine=None):
    h = z["heavy_parts"]
    return (len(h) == 1 and (h[0]["helpers"], h[0]["segments"], h[0]["empty_helpers"]) == (helpers, segments, empty)
            and (fine is None or h[0]["fine_buckets"] == fine) and z["helpers_on"] and not z["Q_above_min"])


PH1 = fm.PH_MIN + 1
PH_H = -(-PH1 // fm.PH_QMIN)  # helpers of a part of PH_MIN + 1 entries (Q = PH_QMIN)
NP16 = 256


def _empty_helpers(S, Hn):
    return sum(S * i // Hn == S * (i + 1) // Hn for i in range(Hn))


def cases():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))
    # ---- tiles: nidx around the digit pass's tile
    for nidx in (1, T - 1, T, T + 1, 2 * T + 1):
        add(f"tiles_{nidx}", "g1", UNSPLIT, lambda nidx=nidx: rand(11, nidx, 128), UNSPLIT_PLAN,
            lambda z, nidx=nidx: z["tiles"] == -(-nidx // T) and z["packed"] and z["part_base"] == {"unrolled", "strided"})
    for n in (1, T // 2, T // 2 + 1, T + 1):
        add(f"tiles_glv_{2 * n}", "g1", GLV, lambda n=n: full_width(12, n, [])[:n], GLV_PLAN,
            lambda z, n=n: z["tiles"] == -(-2 * n // T) and z["source"] == "glv" and z["part_base"] == {"unrolled"},
            bases="plain")
    # ---- register-kept against walked segments: tile 0 holds PS_RK PS_TEAM entries of one part (team 0
    # keeps them), tile 1 one more (team 1 of the same workgroup walks)
    keep = [dig(d, 3) for d in part_digits(5, fm.PS_KEEP)]
    add("kept_96_walked_97", "g1", UNSPLIT, lambda: keep + [0] * (T - len(keep)) + keep + [dig(5 * 128 + 7, 3)],
        UNSPLIT_PLAN, lambda z: (z["teams_kept"], z["teams_walked_long"], z["parts_mixed"], z["tiles"]) == (1, 1, 1, 2))
    add("kept_96", "g1", UNSPLIT, lambda: keep, UNSPLIT_PLAN,
        lambda z: (z["teams_kept"], z["teams_walked_long"], z["teams_walked_many"]) == (1, 0, 0))
    # ---- staged against direct stores: a light part's span at and above the LDS stage
    for k, side in ((fm.PS_STAGE, "staged"), (fm.PS_STAGE + 1, "direct")):
        add(f"span_{side}", "g1", UNSPLIT, lambda k=k: [dig(d, 2) for d in part_digits(9, k)], UNSPLIT_PLAN,
            lambda z, side=side: (z["parts_staged"], z["parts_direct"]) == ((1, 0) if side == "staged" else (0, 1))
            and not z["heavy_parts"])
        add(f"span_{side}_glv", "g1", GLV, lambda k=k: [dig(d, 2) for d in part_digits(9, k)], GLV_PLAN,
            lambda z, side=side: (z["parts_staged"], z["parts_direct"]) == ((1, 0) if side == "staged" else (0, 1))
            and not z["heavy_parts"] and z["source"] == "glv", bases="plain")
    # ---- heavy parts: PH_MIN entries stay light, PH_MIN + 1 get helpers (some with an empty range)
    add("part_at_PH_MIN", "g1", UNSPLIT, lambda: [dig(d, 1) for d in part_digits(3, fm.PH_MIN)], UNSPLIT_PLAN,
        lambda z: not z["heavy_parts"] and z["max_part"] == fm.PH_MIN and z["parts_direct"] == 1)
    s3 = -(-PH1 // T)
    add("part_above_PH_MIN", "g1", UNSPLIT, lambda: [dig(d, 1) for d in part_digits(3, PH1)], UNSPLIT_PLAN,
        lambda z: _heavy1(z, PH_H, s3, _empty_helpers(s3, PH_H), 128) and _empty_helpers(s3, PH_H) > 0
        and z["parts_direct"] == z["parts_staged"] == 0)
    add("heavy_one_fine_bucket", "g1", UNSPLIT, lambda: [dig(d, 1) for d in part_digits(3, PH1, spread=1)], UNSPLIT_PLAN,
        lambda z: _heavy1(z, PH_H, s3, _empty_helpers(s3, PH_H), 1))
    add("heavy_first_part", "g1", UNSPLIT, lambda: [dig(d, 0) for d in part_digits(0, PH1)], UNSPLIT_PLAN,
        lambda z: _heavy1(z, PH_H, s3, _empty_helpers(s3, PH_H)) and z["heavy_parts"][0]["part"] == 0)
    add("heavy_last_part", "g1", UNSPLIT, lambda: [dig(d, 8) for d in part_digits(NP16 - 1, PH1)], UNSPLIT_PLAN,
        lambda z: _heavy1(z, PH_H, s3, _empty_helpers(s3, PH_H)) and z["heavy_parts"][0]["part"] == 9 * NP16 - 1)
    add("two_heavy_parts", "g1", UNSPLIT,
        lambda: [dig(d, 4) for d in part_digits(6, PH1)] + [dig(d, 4) for d in part_digits(7, PH1)], UNSPLIT_PLAN,
        lambda z: [(h["part"], h["first"], h["helpers"]) for h in z["heavy_parts"]] ==
        [(4 * NP16 + 6, 0, PH_H), (4 * NP16 + 7, PH_H, PH_H)])
    # both halves of d (1 + lambda) are d: 2 n entries in one part
    ng = -(-PH1 // 2)
    add("heavy_glv", "g1", GLV, lambda: [d * (1 + pr.GLV_LAMBDA) for d in part_digits(3, ng)], GLV_PLAN,
        lambda z: len(z["heavy_parts"]) == 1 and z["heavy_parts"][0]["total"] == 2 * ng and z["source"] == "glv"
        and z["heavy_parts"][0]["empty_helpers"] > 0, bases="plain")
    # all four quarters of d (1 + x + x^2 + x^3) are d
    nq = -(-PH1 // 4)
    x = pr.PSI_X
    add("heavy_psi", "g2", PSI, lambda: [d * (1 + x + x * x + x ** 3) for d in part_digits(3, nq)], PSI_PLAN,
        lambda z: len(z["heavy_parts"]) == 1 and z["heavy_parts"][0]["total"] == 4 * nq and z["source"] == "psi",
        bases="plain")
    # ---- the same three on the plan a caller gets without asking (auto c: 8 up to 2^13 points, 11 up to 2^15)
    dflt = lambda cc: dict(c=cc, W=-(-128 // cc), Wg=-(-128 // cc), F=1, sF=0, split=2, prepared=0, bstride=1,
                           partition_sort=1, fused_chunk_counts=0, chunk=L)
    for n, cc in ((T // 2, 8), (T // 2 + 1, 11)):
        add(f"tiles_default_{2 * n}", "g1", {}, lambda n=n: full_width(14, n, [])[:n], dflt(cc),
            lambda z, n=n, cc=cc: z["tiles"] == -(-2 * n // T) and z["source"] == "glv" and z["FB"] == max(cc - 9, 0),
            bases="plain")
    for k, side in ((fm.PS_STAGE, "staged"), (fm.PS_STAGE + 1, "direct")):
        add(f"span_{side}_default", "g1", {}, lambda k=k: [dig(d, 2, 11) for d in part_digits(9, k, 11)], dflt(11),
            lambda z, side=side: (z["parts_staged"], z["parts_direct"]) == ((1, 0) if side == "staged" else (0, 1))
            and not z["heavy_parts"] and z["FB"] == 2, bases="plain")
    add("heavy_default", "g1", {}, lambda: [d * (1 + pr.GLV_LAMBDA) for d in part_digits(3, ng, 11)], dflt(11),
        lambda z: len(z["heavy_parts"]) == 1 and z["heavy_parts"][0]["total"] == 2 * ng and z["FB"] == 2
        and z["heavy_parts"][0]["fine_buckets"] == 4, bases="plain")
    # ---- helpers switched off: more than PH_HELPERS / 2 heavy parts.  G1 GLV c = 7 is the one accepted
    # plan with enough parts (19 x 64) and contributions at n <= 2^18: both halves of a + b lambda
    # repeat one of 15 digits in 18 windows, so 18 x 15 parts hold 2^19 / 15 > PH_MIN entries each
    def many_heavy_parts():
        rep = sum(1 << (7 * w) for w in range(18))
        return [(1 + (2 * i) % 15) * rep + (1 + (2 * i + 1) % 15) * rep * pr.GLV_LAMBDA for i in range(1 << 18)]
    assert (1 << 19) // 15 > fm.PH_MIN and 18 * 15 > fm.PH_HELPERS // 2
    add("helpers_off", "g1", dict(c=7), many_heavy_parts,
        dict(c=7, W=19, Wg=19, split=2, prepared=0, partition_sort=1, fused_chunk_counts=0, chunk=1024),
        lambda z: not z["helpers_on"] and z["unhelped_heavy"] == 18 * 15 and not z["heavy_parts"] and
        z["parts_direct"] == 18 * 15 and z["parts_staged"] == 0 and z["heavy_plan"] == "planned", bases="plain")
    # ---- chunk tables, through the fused form (c = 16) and k_chunk_counts (c = 13)
    add("chunks_fused", "g1", UNSPLIT, lambda: layout(CHUNK_SPECS), UNSPLIT_PLAN, lambda z: chunk_cell(z) and z["fused"])
    add("chunks_separate", "g1", UNSPLIT13, lambda: layout(CHUNK_SPECS, c=13), UNSPLIT13_PLAN,
        lambda z: chunk_cell(z) and not z["fused"])
    for cfg, plan, cc, tag in ((UNSPLIT, UNSPLIT_PLAN, 16, "fused"), (UNSPLIT13, UNSPLIT13_PLAN, 13, "separate")):
        add(f"slices_{tag}", "g1", cfg, lambda cc=cc: [dig(1, 0, cc)] * (HS * L) + [dig(1, 1, cc)] * (HS * L + 1), plan,
            lambda z: {(0, HS), (0, HS + 1)} <= z["chunk_cells"] and z["max_slices"] == 2 and z["heavy_buckets"] == 2)
        add(f"one_heavy_bucket_{tag}", "g1", cfg, lambda cc=cc: [dig(77, 2, cc)] * (SM * L + 1), plan,
            lambda z: z["heavy_buckets"] == 1 and z["max_chunks"] == SM + 1)
        add(f"many_heavy_buckets_{tag}", "g1", cfg, lambda cc=cc: many_heavy(cc, 8), plan,
            lambda z: z["heavy_plan"] == "fixed" and z["heavy_buckets"] > fm.HEAVY_LDS and not z["heavy_parts"])
    # ---- empty and tiny
    light = lambda z: z["heavy_plan"] == "none" and not z["heavy_parts"]
    add("one_zero", "g1", UNSPLIT, lambda: [0], UNSPLIT_PLAN, lambda z: light(z) and z["max_chunks"] == 0)
    add("one_one", "g1", UNSPLIT, lambda: [1], UNSPLIT_PLAN, lambda z: light(z) and z["max_chunks"] == 1)
    add("all_zero", "g1", UNSPLIT, lambda: [0] * (T + 1), UNSPLIT_PLAN,
        lambda z: light(z) and z["max_chunks"] == 0 and z["tiles"] == 2 and z["teams_kept"] == 0)
    add("one_among_zeros", "g1", UNSPLIT, lambda: [0] * T + [dig(-5, 6)] + [0] * 9, UNSPLIT_PLAN,
        lambda z: light(z) and z["teams_kept"] == 2 and z["max_chunks"] == 1)
    add("all_zero_glv", "g1", GLV, lambda: [0] * (T // 2 + 1), GLV_PLAN, lambda z: light(z) and z["max_chunks"] == 0,
        bases="plain")
    # ---- digits: all-ones windows (a carry through every window), +B and 1 - B in a middle window
    B = 1 << 15
    add("digit_edges", "g1", UNSPLIT,
        lambda: [(1 << 128) - 1, (1 << 128) - (1 << 16), dig(B, 4), dig(1 - B, 4), dig(B, 8), dig(-1, 0), dig(B, 0) + dig(B, 1),
                 sum(dig(B, w) for w in range(9)), sum((B + 1) << (16 * w) for w in range(8))] + rand(13, 40, 128),
        UNSPLIT_PLAN, light)
    # ---- the plans: random scalars, the splits' boundary scalars, scalars at and above r
    glv_e, psi_e = H.glv_edge_scalars(), H.psi_edge_scalars()
    for cc, W, fused in ((16, 8, 1), (13, 10, 0), (9, 15, 0), (5, 26, 0), (2, 64, 0)):
        add(f"plan_glv_c{cc}", "g1", dict(c=cc), lambda: full_width(20, 300, glv_e),
            dict(c=cc, W=W, Wg=W, split=2, prepared=0, bstride=1, fused_chunk_counts=fused, partition_sort=1),
            lambda z, cc=cc: z["source"] == "glv" and z["index"] == "blocked" and z["NP"] == min(256, 1 << (cc - 1)) and
            z["FB"] == max(cc - 9, 0), bases="plain")
    add("plan_glv_c16_mont", "g1", GLV, lambda: full_width(21, 200, glv_e), GLV_PLAN, lambda z: z["source"] == "glv",
        bases="plain", mont=True)
    for cc, W, fused in ((16, 4, 1), (13, 5, 0)):
        add(f"plan_psi_c{cc}", "g2", dict(c=cc), lambda: full_width(22, 300, psi_e),
            dict(c=cc, W=W, Wg=W, split=4, prepared=0, bstride=1, fused_chunk_counts=fused, partition_sort=1),
            lambda z: z["source"] == "psi" and z["index"] == "blocked", bases="plain")
    add("plan_psi_c16_mont", "g2", PSI, lambda: full_width(23, 200, psi_e), PSI_PLAN, lambda z: z["source"] == "psi",
        bases="plain", mont=True)
    add("plan_g2_192", "g2", dict(c=16, bitsize=192), lambda: rand(24, 500, 192) + [(1 << 192) - 1, 0, 1],
        dict(c=16, W=13, Wg=13, split=1, partition_sort=1, fused_chunk_counts=1),
        lambda z: z["source"] == "plain" and z["sort"] == "partitioned" and z["scans"] == {"loop", "register"})
    add("plan_g1_c18", "g1", dict(c=18, bitsize=128), lambda: rand(25, 500, 128) + [(1 << 128) - 1, 0, 1, dig(1 << 17, 3, 18),
                                                                                  dig(1 - (1 << 17), 3, 18)],
        dict(c=18, W=8, Wg=8, split=1, partition_sort=0, fused_chunk_counts=0), lambda z: z["sort"] == "atomic_rank")
    add("plan_g2_c17", "g2", dict(c=17), lambda: full_width(26, 500, psi_e),
        dict(c=17, W=16, Wg=16, split=1, partition_sort=0, fused_chunk_counts=0), lambda z: z["sort"] == "atomic_rank")
    add("plan_g2_c17_mont", "g2", dict(c=17), lambda: full_width(27, 100, []),
        dict(c=17, W=16, Wg=16, split=1, partition_sort=0), lambda z: z["sort"] == "atomic_rank", mont=True)
    # shift tables: G1 F = 4 has blocks of 64 bits -- c = 16 divides them, c = 13 leaves a 12-bit top window
    shift_e = [(1 << 64) - 1, (1 << 255) - 1, sum(0xfff << (64 * f + 52) for f in range(4)),
               sum(((1 << 64) - 1) << (64 * f) for f in (0, 2)), (1 << 52) - 1 + (0xfff << 52)]
    add("plan_shift_full", "g1", dict(c=16, precompute_factor=4), lambda: full_width(28, 600, shift_e),
        dict(c=16, W=16, Wg=4, F=4, sF=64, split=1, bstride=1, partition_sort=1, fused_chunk_counts=1),
        lambda z: z["source"] == "shift" and not z["narrow_top"])
    add("plan_shift_narrow", "g1", dict(c=13, precompute_factor=4), lambda: full_width(29, 600, shift_e),
        dict(c=13, W=20, Wg=5, F=4, sF=64, split=1, bstride=1, partition_sort=1, fused_chunk_counts=0),
        lambda z: z["source"] == "shift" and z["narrow_top"])
    add("plan_slot0", "g1", dict(precompute_factor=3), lambda: full_width(30, 300, glv_e),
        dict(c=8, W=16, Wg=16, F=1, split=2, prepared=0, bstride=3, partition_sort=1),
        lambda z: z["slot0"] and z["source"] == "glv" and z["index"] == "blocked", bases="table")
    add("plan_prepared_g1", "g1", dict(precompute_factor=2), lambda: full_width(31, 300, glv_e),
        dict(c=8, W=16, Wg=16, F=1, split=2, prepared=1, bstride=1, partition_sort=1), lambda z: z["index"] == "point_major")
    add("plan_prepared_g2", "g2", dict(precompute_factor=4), lambda: full_width(32, 300, psi_e),
        dict(c=11, W=6, Wg=6, F=1, split=4, prepared=1, bstride=1, partition_sort=1), lambda z: z["index"] == "point_major")
    for k in c:
        k.n = len(k.scalars())
    return c


CASES = cases()
BY_NAME = {k.name: k for k in CASES}
assert len(BY_NAME) == len(CASES)
