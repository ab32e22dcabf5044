"""The NTT pass of csrc/ntt.hip (k_ntt_pass, ntt_device) restated in Python integers, and the
closed-form transforms of the structured inputs that drive it to its reduction boundaries.

The model restates the kernel's VALUES, not its memory layout: the same pass plan (npass and
(s0, L, logC) per pass), lazy values in [0, 2r) between the first load and the last store, the
exact radix-2^261 lazy product (x w + m r) / 2^261 with m = -x w r^-1 mod 2^261 on twiddles stored
as w 2^261 mod r (mbls_fr29.hpp), one conditional 2r correction per add / sub, the multiplies
skipped exactly where the kernel skips them (the first stage pair of the first pass, and a lone
first radix-2 stage), reduce_once on the forward's last store and the reducing radix-2^256
product by n^-1 on the inverse's.  It asserts the invariants the kernel's comments claim and
counts how often each exact-boundary case is reached; `mutant=` turns one boundary decision the
wrong way, so a test can show that an input family tells the right kernel from a wrong one.

Everything is an element of Fr in Montgomery form (x 2^256 mod r) unless it says otherwise."""
from __future__ import annotations

import os
import re

import numpy as np

import helpers as H
from helpers import pyref as pr

R = pr.R
TWO_R = 2 * R
W256 = 1 << 256
RP29 = 1 << 261  # Montgomery radix of the butterflies' products
_M261 = RP29 - 1
_RINV261 = pow(R, -1, RP29)
_RINV256 = pow(R, -1, W256)

NTT_HIP = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd", "csrc", "ntt.hip")

MUTANTS = ("reduce_gt",     # reduce_once compares with > instead of >=: r is stored as r
           "add_keep_2r",   # add_2r keeps a sum equal to 2r
           "sub_eq_adds",   # sub_2r adds 2r when a == b
           "add_no_carry")  # add_2r ignores the carry out of 2^256
EVENTS = ("add_eq_2r", "add_carry", "sub_eq", "mul_in_ge_r", "store_eq_r", "store_ge_r")

# log_n of the transforms each GPU test checks against the oracle (H.oracle_ntt): the parameter
# lists are read from here, and test_gpu_ntt.py checks that their union leaves no size out
ORACLE_CHECKED_LOG_N = {
    "test_gpu_parity::test_ntt_vs_oracle": [11, 12, 15, 17, 20],
    "test_gpu_parity::test_ntt_past_init_tables_vs_oracle": [23, 24],
    "test_gpu_parity::test_ntt_batch_and_inplace": [10],
    "test_gpu_parity::test_bench_ntt_2_22_single_and_batch4": [22],
    "test_gpu_ntt::test_structured_families_device": [1, 2, 3, 8, 9, 12, 13, 17],
    "test_gpu_ntt::test_remaining_pass_plans_vs_oracle": [0, 4, 5, 6, 7, 13, 14, 16, 18, 19, 21],
}


def _define(src, name):
    m = re.search(r"#define\s+" + name + r"\s+(\d+)", src)
    assert m, name
    return int(m.group(1))


def kernel_defaults():
    """(MBLS_NTT_TILE_LOG, MBLS_NTT_PASS_STAGES) as ntt.hip defaults them"""
    src = open(NTT_HIP).read()
    return _define(src, "MBLS_NTT_TILE_LOG"), _define(src, "MBLS_NTT_PASS_STAGES")


def plan(log_n, tile_log=None, pass_stages=None):
    """ntt.hip's pass plan (pass_plan): [(s0, L, logC)] for a transform of 2^log_n (log_n >= 1)"""
    if tile_log is None or pass_stages is None:
        tile_log, pass_stages = kernel_defaults()
    npass = (log_n + pass_stages - 1) // pass_stages
    out, s0 = [], 0
    for p in range(npass):
        remaining = log_n - s0
        L = (remaining + (npass - p) - 1) // (npass - p)
        colspace = (log_n - L) if p == 0 else s0
        logC = min(tile_log - L, colspace)
        out.append((s0, L, logC))
        s0 += L
    assert s0 == log_n
    return out


def bitrev_perm(log_n):
    n = 1 << log_n
    rev = np.zeros(n, dtype=np.int64)
    for b in range(log_n):
        rev |= ((np.arange(n) >> b) & 1) << (log_n - 1 - b)
    return rev


class Pass:
    """one transform through the model: .out (canonical unless a mutant broke it) and .ev"""

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.mutant = mutant
        self.ev = dict.fromkeys(EVENTS, 0)

    # ---- the kernel's arithmetic ------------------------------------------------------
    def _lazy(self, v):
        # the [0, 2r) invariant of every value a butterfly stores (a mutant may break it)
        if self.mutant is None:
            assert 0 <= v < TWO_R, hex(v)
        return v

    def add_2r(self, a, b):
        s = a + b
        self.ev["add_eq_2r"] += s == TWO_R
        self.ev["add_carry"] += s >= W256
        carry = s >= W256 and self.mutant != "add_no_carry"
        s &= W256 - 1
        keep = not carry and (s <= TWO_R if self.mutant == "add_keep_2r" else s < TWO_R)
        return self._lazy(s if keep else (s - TWO_R) & (W256 - 1))

    def sub_2r(self, a, b):
        self.ev["sub_eq"] += a == b
        borrow = a <= b if self.mutant == "sub_eq_adds" else a < b
        d = (a - b) & (W256 - 1)
        return self._lazy((d + TWO_R) & (W256 - 1) if borrow else d)

    def mul_words(self, x, w29):
        """r29::mul_words: x < 2^256 words, w29 = w 2^261 mod r canonical -> x w / 2^261, lazy"""
        assert 0 <= x < W256 and 0 <= w29 < R
        self.ev["mul_in_ge_r"] += x >= R
        t = x * w29
        m = (-t * _RINV261) & _M261
        t = (t + m * R) >> 261
        assert t < W256, hex(t)  # the product is taken back as words
        return self._lazy(t)

    def reduce_once(self, v):
        sub = v > R if self.mutant == "reduce_gt" else v >= R
        return v - R if sub else v

    def fr_mul(self, a, b):
        """fips::mul (radix 2^256, reducing): a < 2r, b < r -> canonical"""
        t = a * b
        m = (-t * _RINV256) & (W256 - 1)
        return self.reduce_once((t + m * R) >> 256)

    def put(self, v, scale):
        self.ev["store_eq_r"] += v == R
        self.ev["store_ge_r"] += v >= R
        return self.fr_mul(v, scale) if scale is not None else self.reduce_once(v)

    # ---- the transform ----------------------------------------------------------------
    def run(self, x, inverse=False):
        """x: n canonical Montgomery values (n = 2^log_n); returns the n outputs"""
        n = len(x)
        log_n = n.bit_length() - 1
        assert 1 << log_n == n and all(0 <= v < R for v in x)
        scale = pr.fr_to_mont(pow(n, -1, R)) if inverse else None
        if log_n == 0:  # k_copy_scale, no scaling: n^-1 = 1
            self.out = list(x)
            return self.out
        # w_n^i 2^261 mod r, i < n/2 (k_twiddles: stage s entry j is w_n^(j 2^(log_n - s)))
        w = pr.omega(log_n)
        if inverse:
            w = pow(w, -1, R)
        tw, t = [], RP29 % R
        for _ in range(n // 2):
            tw.append(t)
            t = (t * w) % R
        rev = bitrev_perm(log_n)
        a = [x[int(i)] for i in rev]  # the first pass's gather: DIT order
        passes = plan(log_n)
        for p, (s0, L, _logC) in enumerate(passes):
            first, last = p == 0, p == len(passes) - 1
            l = 1
            while l + 1 <= L:  # stage pairs as 2 x 2 butterflies
                fin = last and l + 2 > L
                self._pair(a, log_n, s0 + l, first and l == 1, tw, scale, fin)
                l += 2
            if l == L:  # odd stage count: one radix-2 stage
                self._stage(a, log_n, s0 + l, not (l > 1 or not first), tw, scale, last)
        self.out = a
        return a

    def _stage(self, a, log_n, s, skip_mul, tw, scale, fin):
        n, half, sh = 1 << log_n, 1 << (s - 1), log_n - s
        for base in range(0, n, 2 * half):
            for j in range(half):
                i0, i1 = base + j, base + j + half
                b = a[i1] if skip_mul else self.mul_words(a[i1], tw[j << sh])
                y0, y1 = self.add_2r(a[i0], b), self.sub_2r(a[i0], b)
                a[i0], a[i1] = (self.put(y0, scale), self.put(y1, scale)) if fin else (y0, y1)

    def _pair(self, a, log_n, s, triv, tw, scale, fin):
        """stages s and s + 1 on rows (q, q + h, q + 2h, q + 3h), h = 2^(s-1)"""
        n, h = 1 << log_n, 1 << (s - 1)
        sh1, sh2 = log_n - s, log_n - s - 1
        for base in range(0, n, 4 * h):
            for j in range(h):
                i0 = base + j
                x0, x1, x2, x3 = a[i0], a[i0 + h], a[i0 + 2 * h], a[i0 + 3 * h]
                if not triv:
                    x1 = self.mul_words(x1, tw[j << sh1])
                    x3 = self.mul_words(x3, tw[j << sh1])
                y0, y1 = self.add_2r(x0, x1), self.sub_2r(x0, x1)
                y2, y3 = self.add_2r(x2, x3), self.sub_2r(x2, x3)
                if not triv:
                    y2 = self.mul_words(y2, tw[j << sh2])
                y3 = self.mul_words(y3, tw[(j + h) << sh2])
                o = (self.add_2r(y0, y2), self.add_2r(y1, y3), self.sub_2r(y0, y2), self.sub_2r(y1, y3))
                if fin:
                    o = tuple(self.put(v, scale) for v in o)
                a[i0], a[i0 + h], a[i0 + 2 * h], a[i0 + 3 * h] = o


def run(x, inverse=False, mutant=None):
    """(outputs, event counters) of one modelled transform"""
    m = Pass(mutant)
    return m.run(list(x), inverse), m.ev


# ----------------------------------------------------------------------------- structured inputs
FIXED_RANDOM = 0x2b5f1c9a7d3e4f60718293a4b5c6d7e8f90a1b2c3d4e5f6071829304a5b6c7d8 % R


class Family:
    """a structured input and its transforms in closed form (pow and running products only):
    .x, .fwd, .inv are lists of n canonical Montgomery values"""

    def __init__(self, name, x, fwd, inv):
        self.name = name
        one = pr.FR_R  # (most closed forms are all zero but for one or two positions)
        self.x, self.fwd, self.inv = ([(v * one) % R if v else 0 for v in t] for t in (x, fwd, inv))

    def expect(self, inverse):
        return self.inv if inverse else self.fwd


def _powers(b, n):
    """[b^i for i < n] by a running product"""
    out, t = [], 1
    for _ in range(n):
        out.append(t)
        t = (t * b) % R
    return out


def families(log_n):
    """every structured family at n = 2^log_n (standard-form reasoning; forward X_j = sum_i x_i
    w^(ij), inverse x_i = n^-1 sum_j X_j w^(-ij)):
      constant c        -> forward n c at 0;            inverse c at 0
      v delta at k      -> forward v w^(kj);            inverse n^-1 v w^(-kj)
      w^(m i)           -> forward n at -m mod n;       inverse 1 at m mod n
    alternating +1, -1 is the frequency n/2; sums follow by linearity"""
    n = 1 << log_n
    w = pr.omega(log_n)
    wi = pow(w, -1, R)
    ninv = pow(n, -1, R)
    zeros = [0] * n
    out = [Family("zeros", zeros, zeros, zeros)]

    def at(pos, v):
        t = [0] * n
        t[pos % n] = v % R
        return t

    for nm, c in (("1", 1), ("r-1", R - 1), ("rand", FIXED_RANDOM)):
        out.append(Family("const_" + nm, [c] * n, at(0, n * c), at(0, c)))
    seen = []
    for k in (0, 1, n // 2, n - 1, (n // 3) | 1):
        k %= n
        if k in seen:
            continue
        seen.append(k)
        f, b = _powers(pow(w, k, R), n), _powers(pow(wi, k, R), n)
        for nm, v in (("1", 1), ("r-1", R - 1)):
            out.append(Family(f"delta_{k}_{nm}", at(k, v), [(v * t) % R for t in f],
                              [(v * ninv % R * t) % R for t in b]))
    out.append(Family("alternating", [1 if i % 2 == 0 else R - 1 for i in range(n)], at(n // 2, n), at(n // 2, 1)))

    def freq(m):
        return _powers(pow(w, m, R), n)

    seen = []
    for m in (1, 5, n - 1, n // 2):
        if m % n in seen:
            continue
        seen.append(m % n)
        out.append(Family(f"freq_{m}", freq(m), at(-m, n), at(m, 1)))
    # 3 w^(2i) + (r - 2) w^(7i)
    m1, m2, c1, c2 = 2, 7, 3, R - 2
    if (m1 - m2) % n:
        two_f = [(a + b) % R for a, b in zip(at(-m1, n * c1), at(-m2, n * c2))]
        two_i = [(a + b) % R for a, b in zip(at(m1, c1), at(m2, c2))]
    else:
        two_f, two_i = at(-m1, n * (c1 + c2)), at(m1, c1 + c2)
    out.append(Family("two_freq", [(c1 * a + c2 * b) % R for a, b in zip(freq(m1), freq(m2))], two_f, two_i))
    return out


def family(log_n, name):
    return next(f for f in families(log_n) if f.name == name)


# ----------------------------------------------------------------------------- array conversion
def to_limbs(vals):
    """ints < 2^256 -> (n, 4) uint64 (the byte route: H.ints_to_limbs is a Python loop per limb)"""
    buf = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(len(vals), 4).astype(np.uint64)


def from_limbs(arr):
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
