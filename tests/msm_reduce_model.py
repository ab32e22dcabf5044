"""Host-only model of the MSM's bucket reduction and window fold (csrc/msm_common.hip
plan_levels, csrc/msm_core.hpp msm_device / k_reduce_scaled* /
k_reduce_tree4 / final_fold), over points written as integers mod r: the multiple of one fixed
base point, 0 the identity.

The model restates three things and nothing else:
  plan      which kernel runs each reduction level of an unsplit plan (make_plan with a bit size
            that keeps the endomorphism split off), its segment length, weight offset and whether
            the level reads U records;
  schedule  the exact order of additions and doublings each kernel makes, with the guards the lane
            kernels put in front of them, classifying every addition as generic / x_inf / y_inf /
            equal / opposite (x the accumulator, y the operand added; x is tested first, as in
            jac_add, wave::jadd and the XYZZ adders) and every doubling as generic / inf;
  designs   bucket tables m[w][d] (the multiple bucket d of window w holds) that steer chosen
            segments of chosen levels into the exceptional classes, and the (multiple, scalar)
            entries that realise a table: scalar (d + 1) 2^(c w) puts its base into bucket d of
            window w and nowhere else.

It does not model the sort, the accumulation, the bucket sums or the heavy-bucket slice plan:
every designed bucket holds one contribution.  tests/test_gpu_msm_exceptional.py pins the plan
and the digits to the library, checks the census the designs reach and their sensitivity to
mutants of the group law, and runs the entries on the device."""
from collections import Counter
from itertools import product

from helpers import pyref

R = pyref.R

# ---- plan (msm_common.hip plan_levels and its macros) ---------------------------------------------
SEG0_LOG = 2          # level 0, one segment per lane
SEGL_LOG_G2 = 1       # G2 lane levels after level 0
ROW_SEG_LOG = 3       # G1 and G2
WAVE_SEG_LOG = 2
LANE_MIN = 32768      # level 0 in lanes from this many chains
LANE_MIN_G2 = 8192    # G2 lane levels after level 0
LANE_LEVELS = {"g1": 1, "g2": 3}
WAVE_MIN = {"g1": 2048, "g2": 8192}
TREE_MAX = 512
MAX_LEVELS = 16

LANE_KINDS = ("r28x", "r28px", "r28pxU")
KINDS = ("r28x", "r28px", "r28pxU", "row1", "rowU", "wave", "tree4", "fold")
TREE_SITES = ("a", "b", "c", "d", "e", "k", "f", "g", "W", "U'")


def plan(group, c, bitsize):
    """the unsplit plan of make_plan(bitsize, c) and the kernel msm_device launches per level"""
    W = (bitsize + 1 + c - 1) // c  # one bit of headroom for the top carry
    B = 1 << (c - 1)
    g2 = group == "g2"
    modes, m = [], B
    while True:
        assert len(modes) < MAX_LEVELS
        lvl = len(modes)
        ll = SEG0_LOG if lvl == 0 else (SEGL_LOG_G2 if g2 else SEG0_LOG)
        lg, mode = ll, "lane"
        lane_chains = ((m + (1 << ll) - 1) >> ll) * W
        lmin = LANE_MIN_G2 if (lvl > 0 and g2) else LANE_MIN
        if lvl >= LANE_LEVELS[group] or lane_chains < lmin:
            row_chains = ((m + (1 << ROW_SEG_LOG) - 1) >> ROW_SEG_LOG) * W
            mode = "row" if row_chains >= WAVE_MIN[group] else "wave"
            lg = ROW_SEG_LOG if mode == "row" else WAVE_SEG_LOG
        modes.append((mode, lg, m))
        mo = (m + (1 << lg) - 1) >> lg
        if mo <= 1:
            break
        m = mo
    levels, raw_in, span = [], modes[0][0] == "lane", 1
    for lvl, (mode, lg, m_in) in enumerate(modes):
        off, has_u, last = (1 if lvl == 0 else 0), lvl > 0, lvl == len(modes) - 1
        m_out = (m_in + (1 << lg) - 1) >> lg
        if raw_in:
            if g2:
                kind = "r28pxU" if has_u else "r28px"
                raw_in = not last and modes[lvl + 1][0] == "lane"
            else:
                assert lvl == 0
                kind, raw_in = "r28x", False
        elif mode == "wave" and lg == 2 and off == 0 and m_out * W <= TREE_MAX:
            kind = "tree4"
        elif mode == "row":
            kind = "rowU" if has_u else "row1"
        else:
            assert mode == "wave", "a shipped plan's lane levels all read raw XYZZ records"
            kind = "wave"
        levels.append(dict(kind=kind, m_in=m_in, seg_log=lg, off=off, has_u=has_u, last=last, m_out=m_out, span=span))
        span <<= lg
    return dict(group=group, c=c, bitsize=bitsize, W=W, Wg=W, B=B, levels=levels)


# ---- schedule ------------------------------------------------------------------------------------
class Sim:
    """the group law on multiples, counting classes; `mutant` = (cell, fault) mishandles one
    census cell (kind, level, phase, class): "equal_inf" (a doubling returns the identity),
    "opposite_dbl" (a cancellation returns the doubled accumulator), "guard" (a lane kernel adds an
    identity R to a live S: the XYZZ product by zz = 0 leaves zz = 0, S becomes the identity)"""

    def __init__(self, mutant=None):
        self.census = Counter()
        self.mutant = mutant

    def _hit(self, key, fault):
        return self.mutant is not None and self.mutant == (key, fault)

    def add(self, where, x, y):
        if x == 0:
            cls, r = "x_inf", y
        elif y == 0:
            cls, r = "y_inf", x
        elif x == y:
            cls, r = "equal", 2 * x % R
        elif (x + y) % R == 0:
            cls, r = "opposite", 0
        else:
            cls, r = "generic", (x + y) % R
        key = where + (cls,)
        self.census[key] += 1
        if cls == "equal" and self._hit(key, "equal_inf"):
            r = 0
        if cls == "opposite" and self._hit(key, "opposite_dbl"):
            r = 2 * x % R
        return r

    def dbl(self, where, x):
        self.census[where + ("inf" if x == 0 else "generic",)] += 1
        return 2 * x % R

    def guarded(self, where, s):
        """a lane kernel skipped S += R because R is the identity; counted when S is live"""
        if s == 0:
            return s
        key = where + ("guard",)
        self.census[key] += 1
        return 0 if self._hit(key, "guard") else s


def _chain(sim, lv, lvl, Vs, Us):
    """k_reduce_scaled<ROW | WAVE>: no guards, every step goes through the adder"""
    k = (lv["kind"], lvl)
    Rr = S = 0
    for t in range(len(Vs) - 1, -1, -1):
        Rr = sim.add(k + ("R+=V",), Rr, Vs[t])
        if t + lv["off"] != 0:
            S = sim.add(k + ("S+=R",), S, Rr)
        if Us is not None:
            S = sim.add(k + ("S+=U",), S, Us[t])
    if not lv["last"]:
        for _ in range(lv["seg_log"]):
            Rr = sim.dbl(k + ("dbl",), Rr)
    return Rr, S


def _lane(sim, lv, lvl, Vs, Us):
    """k_reduce_scaled_r28x / _r28px: identity records never reach the adder (xadd_raw), S += R
    and the doublings of R are guarded by !R.is_inf()"""
    k = (lv["kind"], lvl)
    Rr = S = 0
    for t in range(len(Vs) - 1, -1, -1):
        if Vs[t] != 0:
            Rr = sim.add(k + ("R+=V",), Rr, Vs[t])
        if t + lv["off"] != 0:
            S = sim.add(k + ("S+=R",), S, Rr) if Rr != 0 else sim.guarded(k + ("S+=R",), S)
        if Us is not None and Us[t] != 0:
            S = sim.add(k + ("S+=U",), S, Us[t])
    if not lv["last"] and Rr != 0:
        for _ in range(lv["seg_log"]):
            Rr = sim.dbl(k + ("dbl",), Rr)
    return Rr, S


def _tree4(sim, lv, lvl, Vs, Us):
    """k_reduce_tree4: inputs past the level's end are the identity; ten additions in four steps"""
    k = (lv["kind"], lvl)
    V = list(Vs) + [0] * (4 - len(Vs))
    U = list(Us) + [0] * (4 - len(Us))
    a = sim.add(k + ("a",), V[2], V[3])
    b = sim.add(k + ("b",), U[0], U[1])
    c = sim.add(k + ("c",), U[2], U[3])
    d = sim.add(k + ("d",), V[0], V[1])
    e = sim.add(k + ("e",), a, V[3])
    kk = sim.add(k + ("k",), a, V[1])
    f = sim.add(k + ("f",), b, c)
    g = sim.add(k + ("g",), d, a)
    Wv = sim.add(k + ("W",), kk, e)
    Up = sim.add(k + ("U'",), Wv, f)
    if not lv["last"]:
        for _ in range(2):
            g = sim.dbl(k + ("dbl",), g)
    return g, Up


_SEGMENT = {"r28x": _lane, "r28px": _lane, "r28pxU": _lane, "row1": _chain, "rowU": _chain, "wave": _chain,
            "tree4": _tree4}


def _level(sim, lv, lvl, V, U):
    """one level over sparse inputs {index: multiple != 0}; all-identity segments are replayed
    once per length and counted in bulk"""
    seg, m_in, m_out = 1 << lv["seg_log"], lv["m_in"], lv["m_out"]
    fn = _SEGMENT[lv["kind"]]
    live = {j >> lv["seg_log"] for j in V}
    if U is not None:
        live |= {j >> lv["seg_log"] for j in U}
    Vo, Uo = {}, {}
    for q in sorted(live):
        k0 = q * seg
        cnt = min(seg, m_in - k0)
        Vs = [V.get(k0 + t, 0) for t in range(cnt)]
        Us = [U.get(k0 + t, 0) for t in range(cnt)] if lv["has_u"] else None
        r, s = fn(sim, lv, lvl, Vs, Us)
        if r:
            Vo[q] = r
        if s:
            Uo[q] = s
    # the identity segments: full ones, and the level's short last one
    tail = m_in - (m_out - 1) * seg
    n_tail = 1 if (tail < seg and (m_out - 1) not in live) else 0
    n_full = m_out - len(live) - n_tail
    for cnt, times in ((seg, n_full), (tail, n_tail)):
        if times:
            one = Sim()
            fn(one, lv, lvl, [0] * cnt, [0] * cnt if lv["has_u"] else None)
            for key, v in one.census.items():
                sim.census[key] += v * times
    return Vo, Uo


def window_sum(pl, buckets, mutant=None):
    """(G_w, census) of one window from its buckets {d: multiple}"""
    sim = Sim(mutant)
    V, U = {d: v % R for d, v in buckets.items() if v % R}, None
    for lvl, lv in enumerate(pl["levels"]):
        V, U = _level(sim, lv, lvl, V, U)
    return U.get(0, 0), sim.census


def fold(pl, G, mutant=None):
    """final_fold: acc = G[Wg - 1]; per window below, c doublings and one addition"""
    sim = Sim(mutant)
    acc = G[-1]
    for w in range(pl["Wg"] - 2, -1, -1):
        for _ in range(pl["c"]):
            acc = sim.dbl(("fold", -1, "dbl"), acc)
        acc = sim.add(("fold", -1, "add"), acc, G[w])
    return acc, sim.census


class Table:
    """one designed input: name, plan, buckets m[w] = {d: signed multiple}, the level it aims at
    (-1: the fold).  `result` and `census` replay it; `mutated(cell, fault)` replays it with one
    cell mishandled (only the windows that reach the cell are replayed again)."""

    def __init__(self, name, pl, target):
        self.name, self.pl, self.target = name, pl, target
        self.m = [dict() for _ in range(pl["Wg"])]
        self._base = None

    def put(self, w, d, v):
        assert 0 <= w < self.pl["Wg"] and 0 <= d < self.pl["B"]
        assert ((d + 1) << (self.pl["c"] * w)) < (1 << self.pl["bitsize"]), "scalar wider than the plan's bit size"
        nv = self.m[w].get(d, 0) + v
        if nv:
            self.m[w][d] = nv
        else:
            self.m[w].pop(d, None)
        self._base = None

    def _run(self):
        if self._base is None:
            wins = [window_sum(self.pl, b) for b in self.m]
            acc, fc = fold(self.pl, [g for g, _ in wins])
            self._base = (wins, acc, fc)
        return self._base

    @property
    def result(self):
        return self._run()[1]

    @property
    def census(self):
        wins, _, fc = self._run()
        tot = Counter(fc)
        for _, cs in wins:
            tot.update(cs)
        return tot

    def claims(self):
        """the exceptional cells of the level this table aims at: what it is answerable for.
        The last level writes no V' (Vout is null), so what tree4 computes at d and g there is
        dropped: those additions run but nothing can depend on them."""
        dead = ("d", "g") if self.target == len(self.pl["levels"]) - 1 else ()
        return sorted(k for k, v in self.census.items()
                      if k[1] == self.target and k[3] in ("equal", "opposite", "guard") and v
                      and not (k[0] == "tree4" and k[2] in dead))

    def mutated(self, cell, fault):
        wins, _, _ = self._run()
        mut = (cell, fault)
        G = [window_sum(self.pl, b, mut)[0] if cs.get(cell) else g for b, (g, cs) in zip(self.m, wins)]
        return fold(self.pl, G, mut)[0]

    def entries(self):
        """[(signed multiple, scalar)]: one contribution per non-empty bucket"""
        c = self.pl["c"]
        return [(v, (d + 1) << (c * w)) for w, b in enumerate(self.m) for d, v in sorted(b.items())]


FAULT = {"equal": "equal_inf", "opposite": "opposite_dbl", "guard": "guard"}

# ---- designs -------------------------------------------------------------------------------------
# A level-l input j of window w stands for the buckets [j span, (j + 1) span), span = the product
# of the segment lengths below l:  V_j = span * sum m[d],  U_j = sum (d - j span + 1) m[d].
# Two buckets at the front of the span give any (V, U) = (span s, span a) with small s, a:
#   m[j span] = 2 s - span a,  m[j span + 1] = span a - s      (level 0: m[j] = s, no U)
# so the templates below are written in units of `span`.
_SF = (5, 7, 11, 13, 17, 19, 23, 29)     # generic V fillers by position
_AF = (31, 37, 41, 43, 47, 53, 59, 61)   # generic U fillers


def place(tab, lvl, w, q, s, a):
    """segment q of level lvl, window w: V_t = span s[t], U_t = span a[t] (a ignored at level 0)"""
    lv = tab.pl["levels"][lvl]
    span, k0 = lv["span"], q << lv["seg_log"]
    for t, st in enumerate(s):
        j = k0 + t
        assert j < lv["m_in"]
        if lvl == 0:
            tab.put(w, j, st)
        else:
            tab.put(w, j * span, 2 * st - span * a[t])
            tab.put(w, j * span + 1, span * a[t] - st)


def chain_templates(cnt, has_u):
    """{name: (s, a)} for a chain of cnt inputs walked from t = cnt - 1 down (top = cnt - 1).
    Units of span; the chain state in comments is (R, S) after the step."""
    top = cnt - 1
    out = {}

    def tpl(name, sv=(), av=()):
        s, a = list(_SF[:cnt]), list(_AF[:cnt])
        for t, v in sv:
            if 0 <= t < cnt:
                s[t] = v
        for t, v in av:
            if 0 <= t < cnt:
                a[t] = v
        out[name] = (s, a)

    tpl("generic")
    # R meets V_t: equal (R = 1 then + 1); opposite (R = 1 then - 1: the identity in mid-segment,
    # the chain goes on from it; with 2 inputs Vout doubles the identity); identity inputs before,
    # between and after live ones (and an identity U under a live S)
    tpl("RV_equal", [(top, 1), (top - 1, 1)])
    tpl("RV_opposite", [(top, 1), (top - 1, -1)])
    tpl("gaps", [(top, 0), (top - 1, 1), (top - 2, 0), (0, 0)] if cnt > 2 else [(top, 0), (top - 1, 1)],
        [(top - 1, 0)])
    tpl("all_identity_V", [(t, 0) for t in range(cnt)])
    if has_u:
        # S meets R: after the top step S = 1 + 2 = 3; R = 1 + 2 (equal) or 1 - 4 (opposite)
        tpl("SR_equal", [(top, 1), (top - 1, 2)], [(top, 2)])
        tpl("SR_opposite", [(top, 1), (top - 1, -4)], [(top, 2)])
        # S meets U_t: S = R = 1 at the top, U = 1 / -1
        tpl("SU_equal", [(top, 1)], [(top, 1)])
        tpl("SU_opposite", [(top, 1)], [(top, -1)])
    else:
        # level 0: the empty bucket under the top one leaves S == R; R = 1 - 2 = -S
        tpl("SR_equal", [(top, 1), (top - 1, 0)])
        tpl("SR_opposite", [(top, 1), (top - 1, -2)])
        # further down the chain: (R, S) = (1, 1), (3, 4), then R = 4 / -4
        tpl("SR_equal_low", [(top, 1), (top - 1, 2), (top - 2, 1)])
        tpl("SR_opposite_low", [(top, 1), (top - 1, 2), (top - 2, -7)])
    return out


def _tree_sites(s, a):
    """(x, y) operands of the ten additions of k_reduce_tree4, in units of span"""
    av, b, c, d = s[2] + s[3], a[0] + a[1], a[2] + a[3], s[0] + s[1]
    e, k, f = av + s[3], av + s[1], b + c
    return {"a": (s[2], s[3]), "b": (a[0], a[1]), "c": (a[2], a[3]), "d": (s[0], s[1]), "e": (av, s[3]),
            "k": (av, s[1]), "f": (b, c), "g": (d, av), "W": (k, e), "U'": (k + e, f)}


def _cls(x, y):
    return "x_inf" if x == 0 else "y_inf" if y == 0 else "equal" if x == y else "opposite" if x + y == 0 else "generic"


def tree_templates():
    """{(site, class): (s, a)}: for every addition of the tree and every exceptional class, the
    small assignment (searched once, deterministically) that puts that site in that class with the
    fewest other sites off the generic path"""
    rng = range(-3, 4)
    cands = [(s, _AF[:4]) for s in product(rng, repeat=4)] + [(_SF[:4], a) for a in product(rng, repeat=4)]
    wv = _SF[1] + 2 * _SF[2] + 3 * _SF[3]  # W of the generic s
    cands += [(_SF[:4], (1, 2, 3, sg * wv - 6)) for sg in (1, -1)]
    best = {}
    for s, a in cands:
        cl = {n: _cls(x, y) for n, (x, y) in _tree_sites(s, a).items()}
        others = sum(1 for v in cl.values() if v != "generic")
        cost = (others, sum(abs(v) for v in s + tuple(a)))
        for n, v in cl.items():
            if v != "generic" and ((n, v) not in best or cost < best[(n, v)][0]):
                best[(n, v)] = (cost, (list(s), list(a)))
    return {k: v[1] for k, v in sorted(best.items())}


def chain_tables(pl):
    """per chain level of the plan: one table, one template per window; the template sits alone in
    segment 5 between generic neighbours (segments 4..7: one lane, pair or row of a wave takes the
    side branch) and, in the lane and row levels, in every segment of a whole wave / workgroup"""
    tabs = []
    for lvl, lv in enumerate(pl["levels"]):
        if lv["kind"] == "tree4":
            continue
        seg, m_out, m_in = 1 << lv["seg_log"], lv["m_out"], lv["m_in"]
        tab = Table(f"{pl['group']}-c{pl['c']}-L{lvl}-{lv['kind']}", pl, lvl)
        gen = chain_templates(seg, lv["has_u"])["generic"]
        names = [n for n in chain_templates(seg, lv["has_u"]) if n != "generic"]
        for w, name in enumerate(names):
            if m_out >= 8:
                s, a = chain_templates(seg, lv["has_u"])[name]
                for q in (4, 6, 7):
                    place(tab, lvl, w, q, *gen)
                place(tab, lvl, w, 5, s, a)
                # all of a wave (64 lanes, 32 pairs), of a workgroup's rows (16)
                block = 64 if lv["kind"] in LANE_KINDS else 16 if lv["kind"] in ("row1", "rowU") else 0
                if m_out >= 128:
                    for q in range(64, 64 + block):
                        place(tab, lvl, w, q, s, a)
            else:  # narrow level: the last segment (short when the level's length is no multiple)
                q = m_out - 1
                cnt = m_in - q * seg
                s, a = chain_templates(cnt, lv["has_u"])[name]
                place(tab, lvl, w, q, s, a)
        tabs.append(tab)
    return tabs


def tree_tables(pl):
    """per tree4 level: the (site, class) templates spread over windows and segments 1.. (segment
    0's V' carries weight 0 at the next level); a level of one segment per window takes one
    template per window, rotated by level, and a short last segment (the last level: d and g are
    dead there) templates for b and U'"""
    tabs = []
    tt = tree_templates()
    keys = list(tt)
    for lvl, lv in enumerate(pl["levels"]):
        if lv["kind"] != "tree4":
            continue
        tab = Table(f"{pl['group']}-c{pl['c']}-L{lvl}-tree4", pl, lvl)
        m_out, m_in = lv["m_out"], lv["m_in"]
        wins = min(pl["Wg"] - 1, 24)
        if m_in < 4:  # one short segment: V0, V1, U0, U1 only (U' = V1 + (U0 + U1))
            assert m_in == 2
            # U' equal / opposite, V1 the identity, b cancelling under a live W, then b's classes
            short = [((5, 3), (1, 2)), ((5, 3), (-1, -2)), ((5, 0), (1, 2)), ((5, 3), (1, -1))]
            short += [tt[k] for k in keys if k[0] == "b"]
            for w, (s, a) in enumerate(short[:wins]):
                place(tab, lvl, w, 0, s[:2], a[:2])
        else:
            per = max(1, min(m_out - 1, 5))
            first = 1 if m_out > 1 else 0
            rot = (7 * lvl) % len(keys)
            order = keys[rot:] + keys[:rot]
            for i, k in enumerate(order[:per * wins]):
                place(tab, lvl, i // per, first + i % per, *tt[k])
        tabs.append(tab)
    return tabs


def fold_tables(pl):
    """window sums and the fold.  Window w's sum is set by bucket 0 (weight 1) unless said otherwise."""
    c, Wg = pl["c"], pl["Wg"]
    top = Wg - 2  # the highest window every digit of which fits the bit size
    tabs = []

    t = Table(f"{pl['group']}-c{c}-fold-equal-opposite", pl, -1)
    # acc = 3; 2^c 3 meets 3 2^c (equal: 3 2^(c+1)); then 2^c 3 2^(c+1) meets its negative; the
    # identity is doubled c times and restarts; the low windows are generic
    t.put(top, 0, 3)
    t.put(top - 1, 0, 3 << c)
    t.put(top - 2, 0, -(3 << (2 * c + 1)))
    t.put(top - 3, 0, 5)
    for w in range(top - 3):
        t.put(w, 0, 7 + 2 * w)
    tabs.append(t)

    t = Table(f"{pl['group']}-c{c}-fold-leading-identity", pl, -1)
    # only windows 0..2 hold anything: the identity is doubled c times per window above them
    for w in range(3):
        t.put(w, 1, 11 + w)
    tabs.append(t)

    t = Table(f"{pl['group']}-c{c}-window-identity", pl, -1)
    # window 2 sums to the identity from live buckets (2 * 3 + 3 * -2), the others are generic
    t.put(2, 1, 3)
    t.put(2, 2, -2)
    for w in (0, 1, 3, 4):
        t.put(w, 0, 13 + w)
        t.put(w, 2, 3)
    tabs.append(t)

    t = Table(f"{pl['group']}-c{c}-one-live-window", pl, -1)
    # every window the identity (from live buckets) but window 3
    for w in range(top + 1):
        if w == 3:
            t.put(w, 0, 17)
            t.put(w, 3, 2)
        else:
            t.put(w, 1, 3)
            t.put(w, 2, -2)
    tabs.append(t)

    t = Table(f"{pl['group']}-c{c}-msm-identity-windows", pl, -1)
    # the whole MSM is the identity: every window cancels by itself
    for w in range(top + 1):  # 1 * 2k + 2 * -k
        t.put(w, 0, 2 * (4 + w))
        t.put(w, 1, -(4 + w))
    tabs.append(t)

    t = Table(f"{pl['group']}-c{c}-msm-identity-fold", pl, -1)
    # the whole MSM is the identity through the fold's last addition: G_1 = 9, G_0 = -9 2^c
    t.put(1, 2, 3)
    t.put(0, 0, -(9 << c))
    tabs.append(t)
    return tabs


PLANS = (("g1", 5, 128), ("g1", 13, 128), ("g1", 16, 128), ("g2", 5, 192), ("g2", 16, 192), ("g2", 18, 192))


def all_tables():
    """{plan key: [Table]} for the six designed plans"""
    out = {}
    for key in PLANS:
        pl = plan(*key)
        out[key] = chain_tables(pl) + tree_tables(pl) + fold_tables(pl)
    return out
