"""CPU-only checks of the Fr inner-product entries at the library boundary: the four names are
declared, exported and bound with the right argument counts, the header carries the timing sentence,
every documented argument error comes back before any device work, so also on a machine without a
GPU, and mbls_fr_inner_plan's scratch bytes follow from the geometry it reports."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

HEADER = os.path.join(H.ROOT, "include", "bls12_381_mi355x.h")
PKG = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd")
LIB = os.path.join(PKG, "lib", "libbls12_381_mi355x.so")

NAMES = {"mbls_fr_inner_products": 7, "mbls_fr_multi_eval": 7, "mbls_fr_powers": 5, "mbls_fr_inner_plan": 4}
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
    for name in ("inner_products", "multi_eval", "powers", "inner_plan"):
        assert callable(getattr(amd, name)), name
    text = " ".join(open(HEADER).read().split())
    assert "the columns are witness polynomials: no branch and no address depends on a field value" in text


def test_argument_errors_come_before_any_device_work(amd):
    L, P = amd.lib(), amd._p
    col = np.zeros((8, 4), dtype=np.uint64)
    out = np.zeros((1024 * 16, 4), dtype=np.uint64)
    plan = (ctypes.c_int64 * 12)()
    cols = (ctypes.c_void_p * 1025)(*[P(col)] * 1025)
    vecs = (ctypes.c_void_p * 17)(*[P(col)] * 17)
    hole = (ctypes.c_void_p * 3)(P(col), None, P(col))
    hc = (ctypes.c_void_p * 1025)(*[P(col)] * 1025)  # the last of the most columns, of the most vectors, is null
    hv = (ctypes.c_void_p * 17)(*[P(col)] * 17)
    hc[1023] = hv[15] = None
    c =ctypes.byref(amd.vec_config())
    c2 = ctypes.byref(amd.vec_config(batch_size=2))
    cb = ctypes.byref(amd.vec_config(batch_size=2, columns_batch=True))
    half = (1 << 25) + 1
    PTR, ARG, NOT = amd.INVALID_POINTER, amd.INVALID_ARGUMENT, amd.API_NOT_IMPLEMENTED
    inner, mev, pw, pl = L.mbls_fr_inner_products, L.mbls_fr_multi_eval, L.mbls_fr_powers, L.mbls_fr_inner_plan
    cases = [
        (inner(None, 1, vecs, 1, 8, c, P(out)), PTR),
        (inner(cols, 1, None, 1, 8, c, P(out)), PTR),
        (inner(cols, 1, vecs, 1, 8, None, P(out)), PTR),
        (inner(cols, 1, vecs, 1, 8, c, None), PTR),
        (inner(hole, 3, vecs, 1, 8, c, P(out)), PTR),
        (inner(cols, 2, hole, 2, 8, c, P(out)), PTR),
        (inner(cols, 0, vecs, 1, 8, c, P(out)), ARG),
        (inner(cols, -1, vecs, 1, 8, c, P(out)), ARG),
        (inner(cols, 1025, vecs, 1, 8, c, P(out)), ARG),
        (inner(cols, 1, vecs, 0, 8, c, P(out)), ARG),
        (inner(cols, 1, vecs, 17, 8, c, P(out)), ARG),
        (inner(cols, 1, vecs, 1, 0, c, P(out)), ARG),
        (inner(cols, 1, vecs, 1, MAX + 1, c, P(out)), ARG),
        (mev(None, 1, 8, P(col), 1, c, P(out)), PTR),
        (mev(cols, 1, 8, None, 1, c, P(out)), PTR),
        (mev(cols, 1, 8, P(col), 1, None, P(out)), PTR),
        (mev(cols, 1, 8, P(col), 1, c, None), PTR),
        (mev(hole, 2, 8, P(col), 1, c, P(out)), PTR),
        (mev(cols, 0, 8, P(col), 1, c, P(out)), ARG),
        (mev(cols, 1025, 8, P(col), 1, c, P(out)), ARG),
        (mev(cols, 1, 8, P(col), 0, c, P(out)), ARG),
        (mev(cols, 1, 8, P(col), 17, c, P(out)), ARG),
        (mev(cols, 1, 0, P(col), 1, c, P(out)), ARG),
        (mev(cols, 1, MAX + 1, P(col), 1, c, P(out)), ARG),
        # a full table whose last member is null: alone, then with no rows and with one member too
        # many (both looked at first), then with a fault of the operand after it (looked at later)
        (inner(hc, 1024, vecs, 1, 8, c, P(out)), PTR),
        (inner(cols, 1, hv, 16, 8, c, P(out)), PTR),
        (inner(hc, 1024, vecs, 1, 0, c, P(out)), ARG),
        (inner(cols, 1, hv, 16, 0, c, P(out)), ARG),
        (inner(hc, 1025, vecs, 1, 8, c, P(out)), ARG),
        (inner(cols, 1, hv, 17, 8, c, P(out)), ARG),
        (inner(hc, 1024, vecs, 17, 8, c, P(out)), PTR),
        (mev(hc, 1024, 8, P(col), 1, c, P(out)), PTR),
        (mev(hc, 1024, 0, P(col), 1, c, P(out)), ARG),
        (mev(hc, 1025, 8, P(col), 1, c, P(out)), ARG),
        (mev(hc, 1024, 8, P(col), 17, c, P(out)), PTR),
        (pw(None, None, 8, c, P(out)), PTR),
        (pw(P(col), None, 8, None, P(out)), PTR),
        (pw(P(col), P(col), 8, c, None), PTR),
        (pw(P(col), None, 0, c, P(out)), ARG),
        (pw(P(col), None, MAX + 1, c, P(out)), ARG),
        (pw(P(col), P(col), half, c2, P(out)), ARG),
        (pw(P(col), None, 4, cb, P(out)), NOT),
        (pl(8, 1, 1, None), PTR),
        (pl(0, 1, 1, plan), ARG),
        (pl(MAX + 1, 1, 1, plan), ARG),
        (pl(8, 0, 1, plan), ARG),
        (pl(8, 1025, 1, plan), ARG),
        (pl(8, 1, 0, plan), ARG),
        (pl(8, 1, 17, plan), ARG),
    ]
    for k, (got, want) in enumerate(cases):
        assert got == want, k
    assert not out.any() and not any(plan)


def up256(x):
    return -(-x // 256) * 256


def test_inner_plan_is_self_consistent(amd):
    base = amd.inner_plan(1)
    T, CB, VB = base["tile"], base["CB"], base["VB"]
    assert CB >= 1 and VB >= 1 and base["defer"] >= 1 and T % base["defer"] == 0
    for n in (1, T - 1, T, T + 1, 3 * T + 5, 1 << 20, (1 << 22) + 3, MAX):
        for nc, nv in ((1, 1), (CB, VB), (CB + 1, VB + 1), (32, 3), (1024, 16)):
            p = amd.inner_plan(n, nc, nv)
            assert (p["tile"], p["CB"], p["VB"], p["defer"]) == (T, CB, VB, base["defer"])
            blocks = -(-nc // CB) * -(-nv // VB)
            tiles = -(-n // T)
            assert 1 <= p["groups"] <= p["group_cap"] and p["tiles_per_group"] == -(-tiles // p["group_cap"])
            assert p["groups"] == -(-tiles // p["tiles_per_group"])
            assert (p["tiles_per_group"] > 1) == (n > p["group_cap"] * T)
            assert p["workgroups"] == p["groups"] * blocks <= p["max_workgroups"]
            # the partial sums do not grow with the size: their count is bounded by the cap
            assert p["inner_bytes"] == up256(32 * p["groups"] * nc * nv) + up256(8 * (nc + nv))
            s = p["pow_log"]
            assert 1 << (2 * s) >= n and (s == 0 or 1 << (2 * s - 2) < n)
            tables = up256(32 * nv * ((1 << s) + -(-n // (1 << s))))
            assert p["multi_eval_bytes"] == p["inner_bytes"] + tables + up256(32 * n * nv)
    cap = amd.inner_plan(MAX, 1, 1)["group_cap"]
    for n in (cap * T, MAX // 2, MAX):
        assert amd.inner_plan(n, 1, 1)["inner_bytes"] <= up256(32 * cap) + 256
