"""The contract of the MSM front (msm_front, csrc/msm_common.hip) as an executable check.

The front hands the accumulation and the bucket sums a set of tables: sorted, offsets, nchunks,
chunk_off, owner, first, perm, binbase and the heavy-bucket table H (DESIGN.md "The front's
contract").  check(tables, plan, scalars) asserts what those tables must hold given only the scalars
and the plan -- never the front's own intermediate results (part_tot, seg_cnt, hh, cloc) -- in a
fixed order, and names the first table that breaks (FrontMismatch.table).

census(plan, D) restates, over integers, the decision rules of k_digits_part, part_plan,
helper_range, k_part_sort, k_chunk_owner and scan_wg: which side of each branch every workgroup or
team takes for the signed digits D.  It is what lets a test claim "this case runs the direct-store
path".

Everything is exact integer arithmetic (numpy int64 for digits and indices, Python integers for
scalars).  The constants are read from the sources by regex, so a retune moves the cases or fails
loudly.  tables / plan have the shape bls12_381_amd.msm_front_tables returns."""
import os
import re

import numpy as np

import helpers as H
from helpers import pyref as pr

CSRC = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd", "csrc")
FILL = 0xA5A5A5A5
TABLES = ("sorted", "offsets", "nchunks", "chunk_off", "owner", "first", "perm", "binbase", "H_bucket", "H_first",
          "H_nslices", "H_done", "H_owner", "H_gdone")


def _constants():
    src = open(os.path.join(CSRC, "msm_common.hip")).read() + open(os.path.join(CSRC, "msm_core.hpp")).read()

    def val(text):
        text = text.strip().rstrip(";")
        m = re.fullmatch(r"(\d+)u?\s*<<\s*(\d+)", text)
        if m:
            return int(m.group(1)) << int(m.group(2))
        return int(re.fullmatch(r"(\d+)u?", text).group(1))

    def define(name):
        m = re.search(r"#define\s+" + name + r"\s+(\S+)", src)
        assert m, name
        return val(m.group(1))

    def const(name):
        m = re.search(r"\b" + name + r"\s*=\s*(\d+u?(?:\s*<<\s*\d+)?)\s*[,;]", src)
        assert m, name
        return val(m.group(1))

    k = {n: define(n) for n in ("MBLS_DT_PER", "MBLS_PS_STAGE", "MBLS_PS_TEAM", "MBLS_PS_THREADS", "MBLS_HEAVY_SLICE",
                                "MBLS_CHUNK")}
    k.update({n: const(n) for n in ("DT_THREADS", "PS_RS", "PS_RK", "PH_MIN", "PH_QMIN", "PH_HELPERS", "SMALL_MAX",
                                    "HEAVY_LDS", "DT_MAX_B", "CHUNK_FUSED_SHIFT", "HEAVY_GDONE", "SCAN_REG")})
    k["DT_TILE"] = k["DT_THREADS"] * k["MBLS_DT_PER"]
    k["ORDER_BINS"] = k["SMALL_MAX"] + 1
    return k


K = _constants()
DT_TILE, PS_STAGE, PS_TEAM, PS_THREADS = K["DT_TILE"], K["MBLS_PS_STAGE"], K["MBLS_PS_TEAM"], K["MBLS_PS_THREADS"]
PS_RS, PS_RK, PH_MIN, PH_QMIN, PH_HELPERS = K["PS_RS"], K["PS_RK"], K["PH_MIN"], K["PH_QMIN"], K["PH_HELPERS"]
SMALL_MAX, HEAVY_SLICE, HEAVY_LDS, CHUNK = K["SMALL_MAX"], K["MBLS_HEAVY_SLICE"], K["HEAVY_LDS"], K["MBLS_CHUNK"]
DT_MAX_B, CHUNK_FUSED_SHIFT, HEAVY_GDONE, ORDER_BINS = K["DT_MAX_B"], K["CHUNK_FUSED_SHIFT"], K["HEAVY_GDONE"], K["ORDER_BINS"]
SCAN_REG = K["SCAN_REG"]
PS_KEEP = PS_RK * PS_TEAM  # entries of one segment a team keeps in registers


class FrontMismatch(AssertionError):
    """check() failed; .table names the first table that breaks the contract"""

    def __init__(self, table, what):
        super().__init__(f"{table}: {what}")
        self.table = table


def _need(cond, table, what):
    if not cond:
        raise FrontMismatch(table, what() if callable(what) else what)


def _first_diff(a, b):
    k = int(np.flatnonzero(a != b)[0])
    return f"word {k}: {int(a[k])} against the model's {int(b[k])}"


# ----------------------------------------------------------------------------- the plan's geometry
def points(plan):
    """n, the MSM's size"""
    return plan["pts"] // (plan["split"] if plan["split"] > 1 else plan["F"])


def windows(plan):
    """[(pos, wid)] of window l of a table block (sF > 0), or of the uniform windows (sF == 0)"""
    c, Wg, sF = plan["c"], plan["Wg"], plan["sF"]
    if sF == 0:
        return [(c * l, c) for l in range(Wg)]
    return [(c * l, min(c, sF - c * l)) for l in range(Wg)]


def stream_index(plan, j, i):
    """value index (sorted entry >> 1) of stream j of point i of a split plan"""
    return i * plan["split"] + j if plan["prepared"] else j * points(plan) + i


def split_weight(plan, j):
    return pow(pr.GLV_LAMBDA if plan["split"] == 2 else pr.BLS_Z, j, pr.R)


def scalar_ints(scalars):
    """(n, 4) uint64 limbs (or a sequence of integers) -> object array of Python integers"""
    if isinstance(scalars, np.ndarray) and scalars.dtype != object:
        s = scalars.astype(object)
        return s[:, 0] + (s[:, 1] << 64) + (s[:, 2] << 128) + (s[:, 3] << 192)
    return np.array([int(v) for v in scalars], dtype=object)


def _to_limbs(x, k):
    """non-negative integers below 2^(64 k) -> (len(x), k) uint64, little-endian limbs"""
    raw = b"".join(int(v).to_bytes(8 * k, "little") for v in x)
    return np.frombuffer(raw, dtype="<u8").reshape(len(x), k)


def _from_limbs(a):
    k = a.shape[1]
    raw = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return np.array([int.from_bytes(raw[8 * k * i:8 * k * (i + 1)], "little") for i in range(len(a))], dtype=object)


def _chain(x, plan, wins):
    """signed digits in [1 - B, B] of the non-negative integers x < 2^256 over `wins`, by the carry
    chain (the unique representation with that range where every window is c wide): int64
    (len(x), len(wins)), and the carry out of the last window"""
    c, B = plan["c"], plan["B"]
    limbs = _to_limbs(x, 6)
    out = np.zeros((len(x), len(wins)), dtype=np.int64)
    carry = np.zeros(len(x), dtype=np.int64)
    for l, (pos, wid) in enumerate(wins):
        word, sh = divmod(pos, 64)
        v = limbs[:, word] >> np.uint64(sh)
        if sh + wid > 64:
            v = v | (limbs[:, word + 1] << np.uint64(64 - sh))
        v = (v & np.uint64((1 << wid) - 1)).astype(np.int64) + carry
        carry = (v > B).astype(np.int64)
        out[:, l] = v - (carry << c)
    return out, carry


def _values(D2, wins):
    """sum_l D2[:, l] 2^pos_l as Python integers (object array), for windows that tile
    [0, end) in order: the signed digits are carried into non-negative fields, packed into limbs"""
    end = wins[-1][0] + wins[-1][1]
    assert wins[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(wins, wins[1:]))
    limbs = np.zeros((len(D2), end // 64 + 2), dtype=np.uint64)
    carry = np.zeros(len(D2), dtype=np.int64)
    for l, (pos, wid) in enumerate(wins):
        t = D2[:, l] + carry
        low = t & ((1 << wid) - 1)
        carry = (t - low) >> wid
        word, sh = divmod(pos, 64)
        u = low.astype(np.uint64)
        limbs[:, word] |= u << np.uint64(sh)
        if sh + wid > 64:
            limbs[:, word + 1] |= u >> np.uint64(64 - sh)
    vals = _from_limbs(limbs)
    if carry.any():
        vals = vals + carry.astype(object) * (1 << end)
    return vals


def model_digits(plan, scalars):
    """D[value index, window of the group] = the signed digit, int64 (pts, Wg): from the big-integer
    digits of s mod r (unsplit) or of pr.glv_decompose / pr.psi_decompose's magnitudes (split).
    Uniform windows have one representation in [1 - B, B]; for shift tables this is the carry
    chain's (the front may choose another at a narrow top window)."""
    n, Wg, F, split = points(plan), plan["Wg"], plan["F"], plan["split"]
    s = scalar_ints(scalars) % pr.R
    assert len(s) == n
    D = np.zeros((plan["pts"], Wg), dtype=np.int64)
    if split == 1:
        sF = plan["sF"]
        wins = [(sF * f + pos, wid) for f in range(F) for pos, wid in windows(plan)]
        d, carry = _chain(s, plan, wins)  # the carry runs through all windows in order
        top = s >> (sF * F if sF else plan["c"] * Wg)
        assert not carry.any() and not top.any(), "a scalar outside the plan's windows"
        return d.reshape(n * F, Wg)
    if split == 2:
        parts = [pr.glv_decompose(int(v)) for v in s]  # (m1, neg1, m2, neg2)
        mags, negs = [p[0::2] for p in parts], [p[1::2] for p in parts]
    else:
        parts = [pr.psi_decompose(int(v)) for v in s]  # [(mag, neg)] x 4
        mags, negs = [[m for m, _ in p] for p in parts], [[g for _, g in p] for p in parts]
    mags, negs = np.array(mags, dtype=object).reshape(n, split), np.array(negs, dtype=bool).reshape(n, split)
    if not plan["prepared"]:  # stream_index: j n + i against i split + j
        mags, negs = mags.T, negs.T
    mags, negs = mags.reshape(-1), negs.reshape(-1)
    d, carry = _chain(mags, plan, windows(plan))
    assert not carry.any() and not (mags >> (plan["c"] * Wg)).any(), "a magnitude outside the plan's windows"
    return np.where(negs[:, None], -d, d)


def digit_values(plan, D):
    """the scalar each point's digits stand for: object array (n,), an integer for unsplit plans
    and a residue mod r for split plans"""
    n, Wg, F, split, sF = points(plan), plan["Wg"], plan["F"], plan["split"], plan["sF"]
    if split == 1:
        return _values(D.reshape(n, F * Wg), [(sF * f + pos, wid) for f in range(F) for pos, wid in windows(plan)])
    vals = _values(D, windows(plan))
    vals = vals.reshape(n, split).T if plan["prepared"] else vals.reshape(split, n)
    acc = np.zeros(n, dtype=object)
    for j in range(split):
        acc = acc + vals[j] * split_weight(plan, j)
    return acc % pr.R


# ----------------------------------------------------------------------------- derived tables
def chunk_counts(offsets, TB, L):
    o = offsets[:TB].astype(np.int64)
    cnt = np.diff(offsets[:TB + 1].astype(np.int64))
    return np.where(cnt > 0, (o + cnt - 1) // L - o // L + 1, 0)


def order_slot(b, nch, TB):
    """order_index(block of 256 buckets, bin) of light bucket b with nch chunks (one group)"""
    bpg = (TB + 255) // 256
    return (SMALL_MAX - nch) * bpg + b // 256


def order_words(TB):
    return ORDER_BINS * ((TB + 255) // 256)


def _fill_tail(t, name, start):
    tail = t[start:]
    _need((tail == FILL).all(), name,
          lambda: f"word {start + int(np.flatnonzero(tail != FILL)[0])} past the table's extent was written")


def decode(tables, plan):
    """the sorted table's entries as (bucket, value) arrays, after the offsets checks"""
    TB = plan["TB"]
    off = tables["offsets"][:TB + 1].astype(np.int64)
    _need(off[0] == 0, "offsets", f"offsets[0] = {off[0]}")
    d = np.diff(off)
    _need((d >= 0).all(), "offsets", lambda: f"decreasing at bucket {int(np.flatnonzero(d < 0)[0])}")
    _need(off[TB] <= plan["contributions"], "offsets", f"offsets[TB] = {off[TB]} above the contributions")
    return np.repeat(np.arange(TB, dtype=np.int64), d), tables["sorted"][:off[TB]].astype(np.int64)


def check(tables, plan, scalars, digits=None):
    """assert the front's contract for `tables` (msm_front_tables' dict of arrays) of the MSM of
    `scalars` (standard form: (n, 4) uint64 or integers) under `plan`; raises FrontMismatch.
    digits: model_digits(plan, scalars) where the caller has them already"""
    TB, B, Wg, L = plan["TB"], plan["B"], plan["Wg"], plan["chunk"]
    s = scalar_ints(scalars) % pr.R
    # ---- buckets and offsets
    bucket, val = decode(tables, plan)
    off = tables["offsets"][:TB + 1].astype(np.int64)
    total = int(off[TB])
    idx, sign = val >> 1, val & 1
    _need((idx < plan["pts"]).all(), "sorted", lambda: f"value index {int(idx.max())} of {plan['pts']}")
    key = idx * Wg + bucket // B
    seen = np.bincount(key, minlength=plan["pts"] * Wg)
    _need((seen <= 1).all(), "sorted",
          lambda: "(index, window) %s listed %d times" % (divmod(int(seen.argmax()), Wg), int(seen.max())))
    D = np.zeros(plan["pts"] * Wg, dtype=np.int64)
    D[key] = (bucket % B + 1) * (1 - 2 * sign)  # zero digits cannot be encoded: magnitude = bucket + 1
    D = D.reshape(plan["pts"], Wg)
    want_nz = None
    if plan["sF"] == 0:
        Dm = model_digits(plan, s) if digits is None else digits
        want_nz = int(np.count_nonzero(Dm))
    got = digit_values(plan, D)
    bad = np.flatnonzero(got != s)
    _need(bad.size == 0, "sorted", lambda: f"point {int(bad[0])}: its entries sum to {got[bad[0]]}, the scalar is {s[bad[0]]}")
    if want_nz is not None:
        # ---- exact bucket multisets where the representation is unique: given one entry per
        # (index, window), the buckets' multisets are the model's exactly when the digits are
        bad = np.argwhere(D != Dm)
        _need(bad.size == 0, "sorted",
              lambda: f"index {bad[0][0]} window {bad[0][1]}: digit {D[tuple(bad[0])]}, the model's {Dm[tuple(bad[0])]}")
        _need(total == want_nz, "offsets", f"offsets[TB] = {total}, {want_nz} non-zero digits")
    _fill_tail(tables["sorted"], "sorted", total)
    _fill_tail(tables["offsets"], "offsets", TB + 1)
    # ---- chunk tables
    nch = chunk_counts(tables["offsets"], TB, L)
    got = tables["nchunks"][:TB].astype(np.int64)
    _need((got == nch).all(), "nchunks", lambda: _first_diff(got, nch))
    top = int(nch.max()) if nch.size and nch.max() > 1 else 0
    _need(int(tables["nchunks"][TB]) == top, "nchunks", f"the maximum at [TB] is {int(tables['nchunks'][TB])}, not {top}")
    _fill_tail(tables["nchunks"], "nchunks", TB + 3)
    coff = np.concatenate(([0], np.cumsum(nch)))
    got = tables["chunk_off"][:TB + 1].astype(np.int64)
    _need((got == coff).all(), "chunk_off", lambda: _first_diff(got, coff))
    _fill_tail(tables["chunk_off"], "chunk_off", TB + 1)
    own = np.repeat(np.arange(TB, dtype=np.int64), nch)
    got = tables["owner"][:own.size].astype(np.int64)
    _need((got == own).all(), "owner", lambda: _first_diff(got, own))
    _fill_tail(tables["owner"], "owner", own.size)
    t = (off + L - 1) // L
    fst = np.repeat(np.arange(TB, dtype=np.int64), np.diff(t))
    got = tables["first"][:fst.size].astype(np.int64)
    _need((got == fst).all(), "first", lambda: _first_diff(got, fst))
    _fill_tail(tables["first"], "first", fst.size)
    # ---- order tables
    light = np.flatnonzero(nch <= SMALL_MAX)
    slot = order_slot(light, nch[light], TB)
    ow = order_words(TB)
    base = np.concatenate(([0], np.cumsum(np.bincount(slot, minlength=ow))))
    got = tables["binbase"][:ow + 1].astype(np.int64)
    _need((got == base).all(), "binbase", lambda: _first_diff(got, base))
    perm = tables["perm"][:light.size].astype(np.int64)
    where = np.repeat(np.arange(ow, dtype=np.int64), np.diff(base))
    got = perm[np.lexsort((perm, where))]  # each (block, bin) slice as a set
    want = light[np.lexsort((light, slot))]
    _need((got == want).all(), "perm", lambda: "slice %d of the order: %s" % (int(where[np.flatnonzero(got != want)[0]]),
                                                                             _first_diff(got, want)))
    _fill_tail(tables["perm"], "perm", light.size)
    # ---- heavy table
    heavy = np.flatnonzero(nch > SMALL_MAX)
    nsl = (nch[heavy] + HEAVY_SLICE - 1) // HEAVY_SLICE
    hc, sc = int(tables["nchunks"][TB + 1]), int(tables["nchunks"][TB + 2])
    _need(hc == heavy.size, "H.cnt", f"{hc} heavy buckets listed, {heavy.size} buckets above {SMALL_MAX} chunks")
    _need(sc == int(nsl.sum()), "H.cnt", f"{sc} slices counted, {int(nsl.sum())} wanted")
    hb, hn = tables["H_bucket"][:hc].astype(np.int64), tables["H_nslices"][:hc].astype(np.int64)
    o = np.argsort(hb, kind="stable")
    _need((hb[o] == heavy).all(), "H.bucket", lambda: _first_diff(hb[o], heavy))
    _need((hn[o] == nsl).all(), "H.nslices", lambda: _first_diff(hn[o], nsl))
    hf = tables["H_first"][:hc].astype(np.int64)
    o = np.argsort(hf, kind="stable")
    _need((hf[o] == np.concatenate(([0], np.cumsum(hn[o])))[:hc]).all(), "H.first",
          "the slice ranges do not partition [0, slices)")
    ho = tables["H_owner"][:sc].astype(np.int64)
    want = np.repeat(o, hn[o])
    _need((ho == want).all(), "H.owner", lambda: _first_diff(ho, want))
    _need(not tables["H_done"][:hc].any(), "H.done", "a finished-slices counter is not zero")
    _need(not tables["H_gdone"][:HEAVY_GDONE].any(), "H.gdone", "a group counter is not zero")
    for name, used in (("H_bucket", hc), ("H_first", hc), ("H_nslices", hc), ("H_done", hc), ("H_owner", sc),
                       ("H_gdone", HEAVY_GDONE)):
        _fill_tail(tables[name], name.replace("_", "."), used)
    return D


def complete(plan, entries, off, words):
    """tables that meet the contract's chunk, order and heavy parts for the sorted entries `entries`
    with bucket offsets `off` (TB + 1 words), each table of words[name] words, the rest FILL; heavy
    buckets in bucket order"""
    TB, L = plan["TB"], plan["chunk"]
    off = np.asarray(off, dtype=np.int64)
    t = {name: np.full(words[name], FILL, dtype=np.uint32) for name in TABLES}

    def put(name, arr):
        t[name][:len(arr)] = np.asarray(arr, dtype=np.int64).astype(np.uint32)

    put("sorted", entries)
    put("offsets", off)
    nch = chunk_counts(off, TB, L)
    heavy = np.flatnonzero(nch > SMALL_MAX)
    nsl = (nch[heavy] + HEAVY_SLICE - 1) // HEAVY_SLICE
    put("nchunks", np.concatenate((nch, [nch.max() if nch.max() > 1 else 0, heavy.size, nsl.sum()])))
    put("chunk_off", np.concatenate(([0], np.cumsum(nch))))
    put("owner", np.repeat(np.arange(TB), nch))
    put("first", np.repeat(np.arange(TB), np.diff((off + L - 1) // L)))
    light = np.flatnonzero(nch <= SMALL_MAX)
    slot = order_slot(light, nch[light], TB)
    put("binbase", np.concatenate(([0], np.cumsum(np.bincount(slot, minlength=order_words(TB))))))
    put("perm", light[np.lexsort((light, slot))])
    put("H_bucket", heavy)
    put("H_nslices", nsl)
    put("H_first", np.concatenate(([0], np.cumsum(nsl)))[:heavy.size])
    put("H_done", np.zeros(heavy.size))
    put("H_owner", np.repeat(np.arange(heavy.size), nsl))
    put("H_gdone", np.zeros(HEAVY_GDONE))
    return t


def model_tables(plan, D, words):
    """tables that meet the whole contract for the digits D (pts, Wg): entries in index order inside
    a bucket"""
    idx, wl = np.nonzero(D)
    d = D[idx, wl]
    bucket = wl * plan["B"] + np.abs(d) - 1
    o = np.argsort(bucket, kind="stable")
    off = np.concatenate(([0], np.cumsum(np.bincount(bucket, minlength=plan["TB"]))))
    return complete(plan, ((idx << 1) | (d < 0))[o], off, words)


# ----------------------------------------------------------------------------- the branch census
def sort_sizes(plan):
    """part_sort_sizes: fine bits, parts per window, tiles, packed entries"""
    B = plan["B"]
    lb = B.bit_length() - 1
    FB = lb - 8 if lb > 8 else 0
    nidx = plan["pts"] if plan["split"] > 1 else plan["pts"] // plan["F"]
    return dict(FB=FB, NP=B >> FB, nidx=nidx, tiles=(nidx + DT_TILE - 1) // DT_TILE, pack=plan["pts"] <= 1 << (31 - FB))


def census(plan, D):
    """which side of each of the front's branches the digits D (pts, Wg) take under `plan`"""
    TB, B, Wg, W, F, L = plan["TB"], plan["B"], plan["Wg"], plan["W"], plan["F"], plan["chunk"]
    out = dict(sort="partitioned" if B <= DT_MAX_B else "atomic_rank",
               source=("glv", "psi")[plan["split"] // 4] if plan["split"] > 1 else "shift" if plan["sF"] else "plain",
               narrow_top=bool(plan["sF"] and plan["sF"] % plan["c"]), index="point_major" if plan["prepared"] else
               "blocked" if plan["split"] > 1 else "plain", slot0=plan["bstride"] > 1)
    idx, wl = np.nonzero(D)
    mag = np.abs(D[idx, wl])
    cnt = np.bincount(wl * B + mag - 1, minlength=TB)
    off = np.concatenate(([0], np.cumsum(cnt)))
    # ---- chunk tables (k_chunk_counts or the fused form, k_scan_small, k_chunk_owner)
    nch = chunk_counts(off, TB, L)
    t = (off + L - 1) // L
    queued = (nch > 32) | (np.diff(t) > 32)  # k_chunk_owner: ranges above 32 words go to the workgroup's queue
    heavy = int((nch > SMALL_MAX).sum())
    fused = out["sort"] == "partitioned" and sort_sizes(plan)["FB"] == CHUNK_FUSED_SHIFT
    cs = CHUNK_FUSED_SHIFT if fused else 8
    nblk = (TB + (1 << cs) - 1) >> cs
    out.update(chunk_cells={(int(a), int(b)) for a, b in zip(off[:TB] % L, nch)},
               end_on_chunk=bool(((cnt > 0) & (off[1:] % L == 0)).any()),
               max_chunks=int(nch.max()), owner_queued=int(queued.sum()), owner_direct=int((~queued & (cnt > 0)).sum()),
               heavy_buckets=heavy, heavy_plan="none" if heavy == 0 else "planned" if heavy <= HEAVY_LDS else "fixed",
               max_slices=int(-(-nch.max() // HEAVY_SLICE)) if heavy else 0,
               scans={"register" if (m + 1023) // 1024 <= SCAN_REG else "loop" for m in (order_words(TB), nblk)})
    if out["sort"] != "partitioned":
        return out
    # ---- pass A (k_digits_part): segments (window, tile), parts
    z = sort_sizes(plan)
    FB, NP, tiles = z["FB"], z["NP"], z["tiles"]
    src = idx if plan["split"] > 1 else idx // F  # the digit-source index
    w = wl if plan["split"] > 1 else (idx % F) * Wg + wl
    part = (mag - 1) >> FB
    seg_cnt = np.bincount((w * tiles + src // DT_TILE) * NP + part, minlength=W * tiles * NP).reshape(W, tiles, NP)
    M = Wg * NP
    part_tot = np.array([seg_cnt[g::Wg, :, :].sum(axis=(0, 1)) for g in range(Wg)]).reshape(M)
    PJ = 2048 // PS_THREADS  # k_part_sort's unrolled loads per thread
    # a part's base: workgroup p sums p part totals (block 0 all M), unrolled up to PJ PS_THREADS words
    out.update(fused=fused, packed=z["pack"], tiles=tiles, FB=FB, NP=NP, parts=M, max_part=int(part_tot.max()),
               part_base={"unrolled", "strided"} if M > PJ * PS_THREADS else {"unrolled"})
    # ---- part_plan
    total = int(part_tot.sum())
    thr = max(PH_MIN, 4 * total // M)
    hv = np.flatnonzero(part_tot > thr)
    nh, hs = hv.size, int(part_tot[hv].sum())
    on = 0 < nh <= PH_HELPERS // 2
    Q = max(PH_QMIN, (hs + (PH_HELPERS - nh) - 1) // (PH_HELPERS - nh)) if on else 1
    helped, first = [], 0
    for p in hv if on else []:
        g = int(p) // NP
        S = ((W - 1 - g) // Wg + 1) * tiles
        Hn = (int(part_tot[p]) + Q - 1) // Q
        ranges = [(S * i // Hn, S * (i + 1) // Hn) for i in range(Hn)]
        fine = np.bincount((mag[(wl == g) & (part == int(p) % NP)] - 1) & ((1 << FB) - 1), minlength=1 << FB)
        helped.append(dict(part=int(p), total=int(part_tot[p]), first=first, helpers=Hn, segments=S,
                           empty_helpers=sum(a == b for a, b in ranges), fine_buckets=int((fine > 0).sum())))
        first += Hn
    out.update(heavy_threshold=thr, heavy_parts=helped, helpers_on=on, unhelped_heavy=0 if on else nh, Q=Q,
               Q_above_min=Q > PH_QMIN)
    # ---- pass B (k_part_sort): per team kept in registers or walked, per part staged or direct
    nteams = PS_THREADS // PS_TEAM
    is_helped = np.zeros(M, dtype=bool)
    is_helped[[h["part"] for h in helped]] = True
    kept = walked_long = walked_many = walked_unpacked = mixed = staged = direct = 0
    max_segments = 0
    for p in np.flatnonzero((part_tot > 0) & ~is_helped):
        g = int(p) // NP
        sk = seg_cnt[g::Wg, :, int(p) % NP].reshape(-1)  # segment s = (window of the group, tile)
        S = sk.size
        max_segments = max(max_segments, S)
        pad = np.zeros(-(-S // nteams) * nteams, dtype=np.int64)
        pad[:S] = sk
        pad = pad.reshape(-1, nteams)  # row j: segment team + j nteams
        nseg = np.array([len(range(tm, S, nteams)) for tm in range(nteams)])
        busy = pad.sum(axis=0) > 0
        many = nseg > PS_RS
        long_ = pad.max(axis=0) > PS_KEEP
        keep = z["pack"] & ~many & ~long_
        k, wm, wlg = int((keep & busy).sum()), int((many & busy).sum()), int((~many & long_ & busy).sum())
        kept, walked_many, walked_long = kept + k, walked_many + wm, walked_long + wlg
        walked_unpacked += 0 if z["pack"] else int((~many & ~long_ & busy).sum())
        mixed += bool(k and (wm or wlg))
        if part_tot[p] <= PS_STAGE:
            staged += 1
        else:
            direct += 1
    out.update(teams_kept=kept, teams_walked_long=walked_long, teams_walked_many=walked_many,
               teams_walked_unpacked=walked_unpacked, parts_mixed=mixed,
               parts_staged=staged, parts_direct=direct, max_segments=max_segments,
               segments_per_group=((W - 1) // Wg + 1) * tiles)
    return out
