"""The extended-coset transforms (mbls_fr_coeff_to_extended, mbls_fr_extended_to_coeff; csrc/ntt.hip,
domain section) in Python integers over helpers.pyref.

Everything here is a STANDARD-form residue mod r unless it says otherwise; to_mont_limbs /
from_mont_limbs move lists of them to and from the library's (n, 4) uint64 Montgomery arrays.

  coeff_to_extended(a, N, g)[j]   = sum_{i < len(a)} a[i] (g W^j)^i,                     j < N
  extended_to_coeff(e, N, m, g, vinv)[i] = g^-i N^-1 sum_j e[j] vinv[j mod len(vinv)] W^(-ij), i < m

with W = pr.omega(log2 N).  Direct sums up to DIRECT_MAX points, pr's NTT above (the CPU tests pin
the two routes to each other).  plan() restates mbls_fr_domain_plan on top of ntt_model.plan, and
Halo2Domain restates halo2's EvaluationDomain (extended_k, t_evaluations, distribute_powers_zeta,
coeff_to_extended, divide_by_vanishing_poly, extended_to_coeff)."""
from __future__ import annotations

import ntt_model as NM
from helpers import pyref as pr

R = pr.R
DIRECT_MAX = 1 << 6

# a primitive cube root of unity: halo2's coset generator
ZETA = pow(pr.FR_GENERATOR, (R - 1) // 3, R)
assert pow(ZETA, 3, R) == 1 != ZETA
FIXED_RANDOM = NM.FIXED_RANDOM
GENERATORS = {"one": 1, "zeta": ZETA, "r-1": R - 1, "7": 7, "rand": FIXED_RANDOM}


def log2_exact(n):
    k = n.bit_length() - 1
    assert n >= 1 and 1 << k == n, n
    return k


def next_pow2_log(n):
    return (n - 1).bit_length()


def _powers(b, n):
    out, t = [], 1
    for _ in range(n):
        out.append(t)
        t = (t * b) % R
    return out


# ----------------------------------------------------------------------------- the definitions
def coeff_to_extended(a, N, g=1, direct=None):
    K = log2_exact(N)
    assert 1 <= len(a) <= N
    if direct is None:
        direct = N <= DIRECT_MAX
    if direct:
        W, out = pr.omega(K), []
        x = g % R
        for _ in range(N):
            acc = 0
            for c in reversed(a):  # Horner at x = g W^j
                acc = (acc * x + c) % R
            out.append(acc)
            x = (x * W) % R
        return out
    gp = _powers(g, len(a))
    return pr.ntt_forward([(c * p) % R for c, p in zip(a, gp)] + [0] * (N - len(a)))


def extended_to_coeff(e, N, m, g=1, vinv=None, direct=None):
    K = log2_exact(N)
    assert len(e) == N and 1 <= m <= N
    if vinv is not None:
        assert N % len(vinv) == 0 and len(vinv) & (len(vinv) - 1) == 0
        e = [(v * vinv[j % len(vinv)]) % R for j, v in enumerate(e)]
    gi = pow(g, -1, R)
    if direct is None:
        direct = N <= DIRECT_MAX
    if direct:
        Wi, ninv = pow(pr.omega(K), -1, R), pow(N, -1, R)
        out = []
        for i in range(m):
            x, acc = pow(Wi, i, R), 0
            for v in reversed(e):  # sum_j e[j] x^j
                acc = (acc * x + v) % R
            out.append(acc * ninv % R * pow(gi, i, R) % R)
        return out
    c = pr.ntt_inverse(e)[:m]
    return [(v * p) % R for v, p in zip(c, _powers(gi, m))]


# ----------------------------------------------------------------------------- the plan
PLAN_WORDS = 18


def plan(size, N):
    """mbls_fr_domain_plan's words: dict(passes, E, skipped, rows, fwd_scratch, inv_scratch, plan)"""
    K = log2_exact(N)
    assert 1 <= size <= N
    passes = NM.plan(K) if K else []
    E = K - next_pow2_log(size)
    L0 = passes[0][1] if passes else 0
    skipped = min(E, L0)
    return dict(passes=len(passes), E=E, skipped=skipped, rows=1 << (L0 - skipped), fwd_scratch=0,
                inv_scratch=N if len(passes) > 1 else 0, plan=[tuple(p) for p in passes])


# ----------------------------------------------------------------------------- closed forms
def monomial_extended(v, q, N, g):
    """v X^q -> v g^q W^(qj)"""
    W = pr.omega(log2_exact(N))
    lead = v * pow(g, q, R) % R
    return [(lead * t) % R for t in _powers(pow(W, q, R), N)]


def constant_run_extended(c, size, N, g):
    """c (1 + X + .. + X^(size-1)) -> c ((g W^j)^size - 1) / (g W^j - 1), or c size where g W^j = 1"""
    W = pr.omega(log2_exact(N))
    xs = _powers(W, N)
    xs = [(g * t) % R for t in xs]
    den = [(x - 1) % R for x in xs]
    # one batch inversion (zeros skipped)
    pref, acc = [], 1
    for d in den:
        pref.append(acc)
        if d:
            acc = (acc * d) % R
    inv_all = pow(acc, -1, R)
    inv = [0] * N
    for j in range(N - 1, -1, -1):
        if den[j]:
            inv[j] = (inv_all * pref[j]) % R
            inv_all = (inv_all * den[j]) % R
    return [(c * size) % R if not den[j] else c * (pow(xs[j], size, R) - 1) % R * inv[j] % R for j in range(N)]


# ----------------------------------------------------------------------------- halo2's EvaluationDomain
class Halo2Domain:
    """poly/domain.rs restated: n = 2^k rows, constraint degree j"""

    def __init__(self, k, j):
        self.k, self.n = k, 1 << k
        self.quotient_poly_degree = j - 1
        self.extended_k = k
        while (1 << self.extended_k) < self.n * self.quotient_poly_degree:
            self.extended_k += 1
        self.N = 1 << self.extended_k
        self.extended_omega = pr.omega(self.extended_k)
        self.extended_omega_inv = pow(self.extended_omega, -1, R)
        self.g_coset, self.g_coset_inv = ZETA, (ZETA * ZETA) % R
        assert pow(ZETA, 3, R) == 1 != ZETA
        self.extended_ifft_divisor = pow(self.N, -1, R)
        # 1 / (X^n - 1) on the coset: periodic with 2^(extended_k - k) values
        orig, step = pow(self.g_coset, self.n, R), pow(self.extended_omega, self.n, R)
        t, cur = [], orig
        for _ in range(1 << (self.extended_k - k)):
            t.append(cur)
            cur = (cur * step) % R
        self.t_evaluations = [pow((v - 1) % R, -1, R) for v in t]

    def distribute_powers_zeta(self, a, into_coset):
        coset_powers = [self.g_coset, self.g_coset_inv] if into_coset else [self.g_coset_inv, self.g_coset]
        return [v if i % 3 == 0 else (v * coset_powers[i % 3 - 1]) % R for i, v in enumerate(a)]

    def coeff_to_extended(self, a):
        assert len(a) == self.n
        a = self.distribute_powers_zeta(a, True) + [0] * (self.N - self.n)
        return pr._fft(a, self.extended_omega)

    def divide_by_vanishing_poly(self, a):
        assert len(a) == self.N
        return [(v * self.t_evaluations[i % len(self.t_evaluations)]) % R for i, v in enumerate(a)]

    def extended_to_coeff(self, a):
        assert len(a) == self.N
        a = [(v * self.extended_ifft_divisor) % R for v in pr._fft(a, self.extended_omega_inv)]
        a = self.distribute_powers_zeta(a, False)
        return a[:self.n * self.quotient_poly_degree]


# ----------------------------------------------------------------------------- array conversion
def to_mont_limbs(vals):
    return NM.to_limbs([pr.fr_to_mont(v % R) for v in vals])


def from_mont_limbs(arr):
    return [pr.fr_from_mont(v) for v in NM.from_limbs(arr)]


def mont_words(v):
    """one element as four Montgomery limbs (a coset generator argument)"""
    m = pr.fr_to_mont(v % R)
    return [(m >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]
