"""CPU-only checks of the fixed-base entries at the library boundary: the names are declared, exported
and bound with the right argument counts, the header carries the timing sentence, the plan is
self-consistent, and every documented argument error comes back before any device work, so also on a
machine without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from helpers import pyref as pr

HEADER = os.path.join(H.ROOT, "include", "bls12_381_mi355x.h")
PKG = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd")
LIB = os.path.join(PKG, "lib", "libbls12_381_mi355x.so")

NAMES = {"mbls_fixed_base_plan": 2, "mbls_fixed_base_recode": 2, "mbls_g1_fixed_base_table": 3,
         "mbls_g2_fixed_base_table": 3, "mbls_g1_fixed_base_mul": 6, "mbls_g2_fixed_base_mul": 6,
         "mbls_g1_srs_from_secret": 6}
MAX = 1 << 26


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {name: args.count(",") + 1 for name, args in re.findall(r"^eIcicleError\s+(\w+)\s*\(([^;]*)\);", src, flags=re.M)}


@pytest.fixture(scope="module")
def amd():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", PKG, "-j8", "-s"])
    sys.path.insert(0, PKG)
    import bls12_381_amd
    bls12_381_amd.lib()
    return bls12_381_amd


def test_names_are_declared_exported_and_bound(amd):
    fns = header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for name, nargs in NAMES.items():
        assert fns.get(name) == nargs, name
        assert name in exported, name
        assert name in amd.EXPORTED, name
        f = getattr(amd.lib(), name)
        assert len(f.argtypes) == nargs and f.restype is ctypes.c_int, name
    for name in ("fixed_base_plan", "fixed_base_recode", "fixed_base_table", "fixed_base_mul", "srs_from_secret"):
        assert callable(getattr(amd, name)), name
    text = " ".join(open(HEADER).read().split())
    assert "NOT constant time -- table addresses depend on the scalar's digits" in text
    assert "Do not multiply a secret key, or the secret of a real ceremony, with these calls" in text


def test_plan_is_self_consistent(amd):
    for group, aff, jac in (("g1", 96, 144), ("g2", 192, 288)):
        p = amd.fixed_base_plan(group)
        c, W = p["c"], p["W"]
        assert 2 <= c <= 16
        assert W == -(-255 // c)
        assert p["rows"] == 1 << (c - 1)
        assert p["entries"] == W * p["rows"]
        assert p["entry_bytes"] == aff and p["scratch_per_point"] == jac
        assert p["block"] == 64
        assert p["chunk"] == 0 or (p["chunk"] % p["block"] == 0 and p["chunk"] % 8 == 0)
        # the top digit, with its carry, stays inside a window's rows
        assert ((pr.R - 1) >> (c * (W - 1))) + 1 <= p["rows"]


def test_argument_errors_come_before_any_device_work(amd):
    L, P = amd.lib(), amd._p
    buf = np.zeros((8, 24), dtype=np.uint64)
    out = np.zeros((8, 24), dtype=np.uint64)
    tau = np.array(pr.int_to_limbs(pr.fr_to_mont(5), 4), dtype=np.uint64)
    plan = (ctypes.c_int64 * 8)()
    digits = (ctypes.c_int32 * 64)()
    c = ctypes.byref(amd.vec_config())
    PTR, ARG = amd.INVALID_POINTER, amd.INVALID_ARGUMENT
    pl, rc, srs = L.mbls_fixed_base_plan, L.mbls_fixed_base_recode, L.mbls_g1_srs_from_secret
    cases = [
        (pl(1, None), PTR), (pl(0, plan), ARG), (pl(3, plan), ARG),
        (rc(None, digits), PTR), (rc(P(tau), None), PTR),
    ]
    for tab in (L.mbls_g1_fixed_base_table, L.mbls_g2_fixed_base_table):
        cases += [(tab(None, c, P(out)), PTR), (tab(P(buf), None, P(out)), PTR), (tab(P(buf), c, None), PTR)]
    for mul in (L.mbls_g1_fixed_base_mul, L.mbls_g2_fixed_base_mul):
        cases += [
            (mul(None, P(buf), 8, False, c, P(out)), PTR),
            (mul(P(buf), None, 8, False, c, P(out)), PTR),
            (mul(P(buf), P(buf), 8, False, None, P(out)), PTR),
            (mul(P(buf), P(buf), 8, False, c, None), PTR),
            (mul(P(buf), P(buf), 0, False, c, P(out)), ARG),
            (mul(P(buf), P(buf), -1, True, c, P(out)), ARG),
            (mul(P(buf), P(buf), MAX + 1, False, c, P(out)), ARG),
        ]
    w8 = np.array(pr.int_to_limbs(pr.fr_to_mont(pow(pr.omega(3), 3, pr.R)), 4), dtype=np.uint64)
    one = np.array(pr.int_to_limbs(pr.fr_to_mont(1), 4), dtype=np.uint64)
    w8_unreduced = np.array(pr.int_to_limbs(pr.fr_to_mont(pow(pr.omega(3), 3, pr.R)) + pr.R, 4), dtype=np.uint64)
    cases += [
        (srs(None, P(tau), 8, 0, c, P(out)), PTR),
        (srs(P(buf), None, 8, 0, c, P(out)), PTR),
        (srs(P(buf), P(tau), 8, 0, None, P(out)), PTR),
        (srs(P(buf), P(tau), 8, 0, c, None), PTR),
        (srs(P(buf), P(tau), 0, 0, c, P(out)), ARG),
        (srs(P(buf), P(tau), -8, 1, c, P(out)), ARG),
        (srs(P(buf), P(tau), MAX + 1, 0, c, P(out)), ARG),
        (srs(P(buf), P(tau), 2 * MAX, 1, c, P(out)), ARG),
        (srs(P(buf), P(tau), 8, 2, c, P(out)), ARG),
        (srs(P(buf), P(tau), 8, -1, c, P(out)), ARG),
        (srs(P(buf), P(tau), 6, 1, c, P(out)), ARG),      # basis 1: a power of two
        (srs(P(buf), P(tau), 96, 1, c, P(out)), ARG),
        (srs(P(buf), P(w8), 8, 1, c, P(out)), ARG),       # tau^8 = 1: the pole
        (srs(P(buf), P(w8), 16, 1, c, P(out)), ARG),
        (srs(P(buf), P(one), 1, 1, c, P(out)), ARG),      # n = 1: the only root is 1
        (srs(P(buf), P(one), 4, 1, c, P(out)), ARG),
        (srs(P(buf), P(w8_unreduced), 8, 1, c, P(out)), ARG),  # tau is reduced first
    ]
    for k, (got, want) in enumerate(cases):
        assert got == want, k
    assert not out.any() and not any(plan)
