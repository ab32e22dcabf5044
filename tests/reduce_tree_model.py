"""Host-only model of G1's level-1 reduction tree (csrc/msm_core.hpp reduce_tree8 /
k_reduce_tree8_r28x), over points written as integers mod r: the multiple of one fixed base point,
0 the identity.  It extends tests/msm_reduce_model.py (imported, not changed): the plan, the other
levels' schedules, the fold and the bucket designs are that module's; this one restates what the
device runs at level 1 of a G1 plan whose level 0 runs in lanes and whose level 1 is a row level of
8-input segments (kind "tree8" here, "rowU" there).

The tree.  Eight lanes own one segment; lane j enters with V_j, U_j (the identity past the level's
end).  With P_i = V_2i + V_2i+1 and Q_i = U_2i+1 + U_2i the six passes are
  0 add: P0..P3, Q0..Q3
  1 add: P01 = P0 + P1, T1 = P1 + P3, T2 = P2 + P3, Q01 = Q0 + Q1, Q23 = Q2 + Q3,
         O01 = V3 + V1, O23 = V7 + V5
  2 add: SV = P01 + T2, T12 = T1 + T2, T0 = O01 + O23, SU = Q01 + Q23
  3 add: W = T12 + T2, E = SU + T0;  dbl: 2SV
  4                                  dbl: 2W, 4SV
  5 add: U' = E + 2W;                dbl: V' = 8SV
Every addition is X += b with X the lane's own value and b the value fetched from another lane: b
the identity never reaches the adder (class `y_inf`, X stays), X the identity takes b (`x_inf`),
then equal / opposite / generic as in r28::xadd.  A doubling is skipped when X is the identity
(class `inf`: the guard that keeps zz exactly 0).  The last level writes no V'.

Mutants: "equal_inf" and "opposite_dbl" as in msm_reduce_model.Sim; "dbl_guard" drops the guard of
one doubling site, and the doubled identity goes on as a live point (multiple 1)."""
from math import gcd

import msm_reduce_model as M
from helpers import pyref

R = pyref.R
KEY = ("g1", 16, 128)  # the unsplit plan the designed tables run: 9 windows, level 1 in 1024 segments of 8

ADD_SITES = ("P0", "P1", "P2", "P3", "Q0", "Q1", "Q2", "Q3", "P01", "T1", "T2", "Q01", "Q23", "O01", "O23",
             "SV", "T12", "T0", "SU", "W", "E", "U'")
DBL_SITES = ("2SV", "2W", "4SV", "8SV")
ADD_CLASSES = ("generic", "x_inf", "y_inf", "equal", "opposite")
FAULT = {"equal": "equal_inf", "opposite": "opposite_dbl", "inf": "dbl_guard"}


class Sim(M.Sim):
    def tadd(self, where, x, y):
        """X += b behind the kernel's !b.is_inf() test"""
        if y == 0:
            self.census[where + ("y_inf",)] += 1
            return x
        return self.add(where, x, y)

    def tdbl(self, where, x):
        """the guarded doubling"""
        if x == 0:
            key = where + ("inf",)
            self.census[key] += 1
            return 1 if self._hit(key, "dbl_guard") else 0
        self.census[where + ("generic",)] += 1
        return 2 * x % R


def tree_sites(V, U):
    """the operands (x, y) of the 22 additions and the arguments of the 4 doublings, in the
    kernel's order, as functions of the eight inputs -- over plain integers (design algebra)"""
    P = [V[2 * i] + V[2 * i + 1] for i in range(4)]
    Q = [U[2 * i + 1] + U[2 * i] for i in range(4)]
    s = {f"P{i}": (V[2 * i], V[2 * i + 1]) for i in range(4)}
    s.update({f"Q{i}": (U[2 * i + 1], U[2 * i]) for i in range(4)})
    P01, T1, T2, Q01, Q23, O01, O23 = P[0] + P[1], P[1] + P[3], P[2] + P[3], Q[0] + Q[1], Q[2] + Q[3], V[3] + V[1], \
        V[7] + V[5]
    s.update({"P01": (P[0], P[1]), "T1": (P[1], P[3]), "T2": (P[2], P[3]), "Q01": (Q[0], Q[1]), "Q23": (Q[2], Q[3]),
              "O01": (V[3], V[1]), "O23": (V[7], V[5])})
    SV, T12, T0, SU = P01 + T2, T1 + T2, O01 + O23, Q01 + Q23
    s.update({"SV": (P01, T2), "T12": (T1, T2), "T0": (O01, O23), "SU": (Q01, Q23)})
    W, E = T12 + T2, SU + T0
    s.update({"W": (T12, T2), "E": (SU, T0), "U'": (E, 2 * W)})
    d = {"2SV": SV, "2W": W, "4SV": 2 * SV, "8SV": 4 * SV}
    return s, d


def tree8(sim, lv, lvl, Vs, Us):
    """one segment as the device runs it; returns (V', U')"""
    k = ("tree8", lvl)
    V = list(Vs) + [0] * (8 - len(Vs))
    U = list(Us) + [0] * (8 - len(Us))
    a = lambda n, x, y: sim.tadd(k + (n,), x, y)
    P = [a(f"P{i}", V[2 * i], V[2 * i + 1]) for i in range(4)]
    Q = [a(f"Q{i}", U[2 * i + 1], U[2 * i]) for i in range(4)]
    P01, T1, T2 = a("P01", P[0], P[1]), a("T1", P[1], P[3]), a("T2", P[2], P[3])
    Q01, Q23 = a("Q01", Q[0], Q[1]), a("Q23", Q[2], Q[3])
    O01, O23 = a("O01", V[3], V[1]), a("O23", V[7], V[5])
    SV, T12, T0, SU = a("SV", P01, T2), a("T12", T1, T2), a("T0", O01, O23), a("SU", Q01, Q23)
    W, E = a("W", T12, T2), a("E", SU, T0)
    SV = sim.tdbl(k + ("2SV",), SV)
    W = sim.tdbl(k + ("2W",), W)
    SV = sim.tdbl(k + ("4SV",), SV)
    Up = a("U'", E, W)
    SV = sim.tdbl(k + ("8SV",), SV)
    return SV, Up


def plan(group="g1", c=16, bitsize=128):
    """msm_reduce_model.plan with the level the tree takes renamed: level 1, row mode, segments of
    8, behind a lane level 0 (G1 only)"""
    pl = M.plan(group, c, bitsize)
    lv = pl["levels"]
    if group == "g1" and len(lv) > 1 and lv[0]["kind"] == "r28x" and lv[1]["kind"] == "rowU" and lv[1]["seg_log"] == 3:
        lv[1]["kind"] = "tree8"
    return pl


def library_levels(sched):
    """(kind, seg_log, m_in) per level of the library's own schedule (bls12_381_amd.msm_reduce_plan),
    its (kernel, mode, level > 0) written in this model's kind names -- the form of plan()["levels"].
    A lane level on the generic chain has no kind here ("laneJ": no shipped plan has one)."""
    chain = {"lane": ("laneJ", "laneJ"), "row": ("row1", "rowU"), "wave": ("wave", "wave")}
    out = []
    for lvl, lv in enumerate(sched["levels"]):
        kind = {"chain": chain[lv["mode"]], "tree4": ("tree4", "tree4"), "r28x": ("r28x", None),
                "tree8": ("r28x", "tree8"), "r28px": ("r28px", "r28pxU")}[lv["kernel"]][min(lvl, 1)]
        out.append((kind, lv["seg_log"], lv["m_in"]))
    return out


def model_levels(pl):
    """plan()["levels"] in library_levels' form"""
    return [(lv["kind"], lv["seg_log"], lv["m_in"]) for lv in pl["levels"]]


def _segment(kind):
    return tree8 if kind == "tree8" else M._SEGMENT[kind]


def _level(sim, lv, lvl, V, U):
    """msm_reduce_model._level with the tree's segments (sparse inputs, identity segments in bulk)"""
    if lv["kind"] != "tree8":
        return M._level(sim, lv, lvl, V, U)
    seg, m_in, m_out = 8, lv["m_in"], lv["m_out"]
    live = {j >> 3 for j in V} | {j >> 3 for j in U}
    Vo, Uo = {}, {}
    for q in sorted(live):
        cnt = min(seg, m_in - q * seg)
        r, s = tree8(sim, lv, lvl, [V.get(q * seg + t, 0) for t in range(cnt)],
                     [U.get(q * seg + t, 0) for t in range(cnt)])
        if r:
            Vo[q] = r
        if s:
            Uo[q] = s
    one = Sim()
    tree8(one, lv, lvl, [0] * 8, [0] * 8)  # an identity segment, short or full, runs the same sites
    for key, v in one.census.items():
        sim.census[key] += v * (m_out - len(live))
    return Vo, Uo


def window_sum(pl, buckets, mutant=None):
    sim = Sim(mutant)
    V, U = {d: v % R for d, v in buckets.items() if v % R}, None
    for lvl, lv in enumerate(pl["levels"]):
        V, U = _level(sim, lv, lvl, V, U)
    return U.get(0, 0), sim.census


class Table(M.Table):
    """msm_reduce_model.Table replayed through the tree at level 1"""

    def _run(self):
        if self._base is None:
            wins = [window_sum(self.pl, b) for b in self.m]
            acc, fc = M.fold(self.pl, [g for g, _ in wins])
            self._base = (wins, acc, fc)
        return self._base

    def claims(self):
        """the tree's exceptional cells this table is answerable for: equal / opposite additions
        and guarded doublings of the identity, in segments it placed (an all-identity segment
        reaches the doubling guards too, but nothing there can tell)"""
        return sorted(k for k, v in self.census.items()
                      if k[0] == "tree8" and k[3] in ("equal", "opposite", "inf") and v and k in self.steered)

    def mutated(self, cell, fault):
        wins, _, _ = self._run()
        mut = (cell, fault)
        G = [window_sum(self.pl, b, mut)[0] if cs.get(cell) else g for b, (g, cs) in zip(self.m, wins)]
        return M.fold(self.pl, G, mut)[0]


# ---- designs -------------------------------------------------------------------------------------
# Inputs in units of the level's span (4 buckets): V_j = 4 s[j], U_j = 4 a[j] (msm_reduce_model.place).
GEN_S, GEN_A = M._SF, M._AF  # the generic segment: every site generic


def _solve(form_of, fix=()):
    """inputs (s, a) near the generic ones with form_of(V, U) == 0: the form is linear, so one
    input with coefficient +-1 that is not in `fix` is moved"""
    base = list(GEN_S) + list(GEN_A)
    f0 = form_of(base[:8], base[8:])
    co = []
    for i in range(16):
        e = list(base)
        e[i] += 1
        co.append(form_of(e[:8], e[8:]) - f0)
    g = gcd(*co)  # 2 W = 0 is W = 0: the form's content carries no condition
    for i in range(16):
        if i not in fix and abs(co[i]) == g:
            e = list(base)
            e[i] = -(f0 - co[i] * base[i]) // co[i]  # exact: every coefficient is a multiple of g
            assert form_of(e[:8], e[8:]) == 0
            return e[:8], e[8:]
    raise AssertionError("no coefficient equal to the form's content")


def templates():
    """{(site, class): (s, a)} for every addition site x {x_inf, y_inf, equal, opposite} and every
    doubling site x {inf}: the generic segment with one input moved so that the site's operands
    coincide"""
    out = {}
    for site in ADD_SITES:
        forms = {"x_inf": lambda V, U: tree_sites(V, U)[0][site][0],
                 "y_inf": lambda V, U: tree_sites(V, U)[0][site][1],
                 "equal": lambda V, U: tree_sites(V, U)[0][site][0] - tree_sites(V, U)[0][site][1],
                 "opposite": lambda V, U: tree_sites(V, U)[0][site][0] + tree_sites(V, U)[0][site][1]}
        for cls, f in forms.items():
            out[(site, cls)] = _solve(f)
    for site in DBL_SITES:
        out[(site, "inf")] = _solve(lambda V, U: tree_sites(V, U)[1][site])
    return out


def classify(s, a):
    """{site: class} of one segment"""
    sim = Sim()
    tree8(sim, None, 1, [4 * v % R for v in s], [4 * v % R for v in a])
    return {k[2]: k[3] for k in sim.census}


def tables(pl=None):
    """the designed tables of the tree level, on the unsplit c = 16 plan:
      cells       every template alone in segment 8 i + 5 of a window, the other seven segments of
                  its wave (8 lanes each) generic; templates dealt over windows 0..7
      wave        one template (W equal: T1 = 0) in all eight segments of one wave, and the U'
                  opposite template in all eight of another wave
      tail        identity inputs: a segment with only inputs 0..2 live (the shape of a short last
                  segment: the level itself has 8192 inputs, a multiple of 8), one with only U live
      identity    window 2 sums to the identity through the tree, its neighbours are generic"""
    pl = pl or plan(*KEY)
    assert pl["levels"][1]["kind"] == "tree8"
    tt = templates()
    tabs = []
    wins = pl["Wg"] - 1  # every digit of the top window would pass the bit size

    t = Table("g1-c16-L1-tree8-cells", pl, 1)
    t.steered = set()
    for i, (cell, (s, a)) in enumerate(sorted(tt.items())):
        w, blk = i % wins, 1 + i // wins  # wave `blk` of window w: segments 8 blk .. 8 blk + 7
        for q in range(8 * blk, 8 * blk + 8):
            M.place(t, 1, w, q, *((s, a) if q == 8 * blk + 5 else (GEN_S, GEN_A)))
        t.steered.add(("tree8", 1) + cell)
    tabs.append(t)

    t = Table("g1-c16-L1-tree8-wave", pl, 1)
    t.steered = {("tree8", 1, "W", "equal"), ("tree8", 1, "U'", "opposite")}
    for w, cell in ((0, ("W", "equal")), (1, ("U'", "opposite"))):
        for q in range(16, 24):
            M.place(t, 1, w, q, *tt[cell])
        for q in range(24, 32):
            M.place(t, 1, w, q, GEN_S, GEN_A)
    tabs.append(t)

    t = Table("g1-c16-L1-tree8-tail", pl, 1)
    t.steered = set()
    M.place(t, 1, 0, 9, GEN_S[:3], GEN_A[:3])
    M.place(t, 1, 0, 10, GEN_S, GEN_A)
    M.place(t, 1, 1, 9, [0] * 8, GEN_A)
    M.place(t, 1, 1, 11, GEN_S, [0] * 8)
    M.place(t, 1, 2, pl["levels"][1]["m_out"] - 1, GEN_S, GEN_A)  # the level's last segment
    tabs.append(t)

    t = Table("g1-c16-L1-tree8-window-identity", pl, 1)
    t.steered = set()
    # segment q = 3 of window 2: U' = 4 (sum a + sum j s), V' = 32 sum s, G_w = U' + 8 q V' at the
    # levels above (weight q of 8-input segments: 8 q sum s in units of span) -- cancelled by one
    # input of segment 0 (weight 0: only its U counts)
    s, a = list(GEN_S), list(GEN_A)
    tot = sum(a) + sum(j * v for j, v in enumerate(s)) + 8 * 3 * sum(s)
    M.place(t, 1, 2, 3, s, a)
    M.place(t, 1, 2, 0, [0], [-tot])
    for w in (1, 3):
        M.place(t, 1, w, 3, s, a)
    tabs.append(t)
    return tabs
