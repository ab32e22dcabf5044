"""CPU-only checks of the log-derivative lookup entries at the library boundary: the three names are
declared, exported and bound with the right argument counts, and every documented argument error
comes back before any device work, so also on a machine without a GPU."""
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

NAMES = {"mbls_fr_lookup_multiplicities": 9, "mbls_fr_prefix_sum": 7, "mbls_fr_logup_sum": 10}
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
    for name in ("lookup_multiplicities", "prefix_sum", "logup_sum"):
        assert callable(getattr(amd, name)), name
    text = open(HEADER).read()
    assert "mbls_fr_lookup_multiplicities is NOT constant time" in text


def test_argument_errors_come_before_any_device_work(amd):
    L, P = amd.lib(), amd._p
    col = np.zeros((8, 4), dtype=np.uint64)
    tab = np.zeros((8, 4), dtype=np.uint64)
    m = np.zeros((8, 4), dtype=np.uint64)
    out = np.zeros((8, 4), dtype=np.uint64)
    one = np.zeros((2, 4), dtype=np.uint64)
    cnt = (ctypes.c_uint64 * 2)()
    cols = (ctypes.c_void_p * 65)(*[P(col)] * 65)
    hole = (ctypes.c_void_p * 3)(P(col), None, P(col))
    full = (ctypes.c_void_p * 65)(*[P(col)] * 65)  # the last of the most inputs is null
    full[63] = None
    c = ctypes.byref(amd.vec_config())
    c2 = ctypes.byref(amd.vec_config(batch_size=2))
    cb = ctypes.byref(amd.vec_config(batch_size=2, columns_batch=True))
    half = (1 << 25) + 1
    PTR, ARG, NOT = amd.INVALID_POINTER, amd.INVALID_ARGUMENT, amd.API_NOT_IMPLEMENTED
    mult, psum, lsum = L.mbls_fr_lookup_multiplicities, L.mbls_fr_prefix_sum, L.mbls_fr_logup_sum
    cases = [
        (mult(None, 1, P(tab), 8, True, False, c, P(m), cnt), PTR),
        (mult(cols, 1, None, 8, True, False, c, P(m), cnt), PTR),
        (mult(cols, 1, P(tab), 8, True, False, None, P(m), cnt), PTR),
        (mult(cols, 1, P(tab), 8, True, False, c, None, cnt), PTR),
        (mult(hole, 3, P(tab), 8, True, True, c, P(m), None), PTR),
        (mult(cols, 0, P(tab), 8, True, False, c, P(m), cnt), ARG),
        (mult(cols, -1, P(tab), 8, False, False, c, P(m), cnt), ARG),
        (mult(cols, 65, P(tab), 8, True, False, c, P(m), cnt), ARG),
        (mult(cols, 1, P(tab), 0, True, False, c, P(m), cnt), ARG),
        (mult(cols, 1, P(tab), MAX + 1, True, False, c, P(m), None), ARG),
        (mult(cols, 2, P(tab), half, True, True, c2, P(m), cnt), ARG),
        (mult(cols, 1, P(tab), 4, True, False, cb, P(m), cnt), NOT),
        (psum(None, 8, None, False, c, P(out), None), PTR),
        (psum(P(col), 8, None, False, None, P(out), None), PTR),
        (psum(P(col), 8, None, True, c, None, P(one)), PTR),
        (psum(P(col), 0, None, False, c, P(out), None), ARG),
        (psum(P(col), MAX + 1, None, False, c, P(out), None), ARG),
        (psum(P(col), half, P(one), False, c2, P(out), P(one)), ARG),
        (psum(P(col), 4, None, False, cb, P(out), None), NOT),
        (lsum(None, 1, P(tab), P(m), 8, P(one), None, c, P(out), None), PTR),
        (lsum(cols, 1, None, P(m), 8, P(one), None, c, P(out), None), PTR),
        (lsum(cols, 1, P(tab), None, 8, P(one), None, c, P(out), None), PTR),
        (lsum(cols, 1, P(tab), P(m), 8, None, None, c, P(out), None), PTR),
        (lsum(cols, 1, P(tab), P(m), 8, P(one), None, None, P(out), None), PTR),
        (lsum(cols, 1, P(tab), P(m), 8, P(one), None, c, None, P(one)), PTR),
        (lsum(hole, 2, P(tab), P(m), 8, P(one), None, c, P(out), None), PTR),
        (lsum(cols, 0, P(tab), P(m), 8, P(one), None, c, P(out), None), ARG),
        (lsum(cols, 65, P(tab), P(m), 8, P(one), None, c, P(out), None), ARG),
        (lsum(cols, 1, P(tab), P(m), 0, P(one), None, c, P(out), None), ARG),
        (lsum(cols, 1, P(tab), P(m), MAX + 1, P(one), None, c, P(out), None), ARG),
        (lsum(cols, 4, P(tab), P(m), half, P(one), P(one), c2, P(out), P(one)), ARG),
        (lsum(cols, 1, P(tab), P(m), 4, P(one), None, cb, P(out), None), NOT),
        # a full table whose last member is null: alone, then with no rows and with one input too
        # many, both of which are looked at first
        (mult(full, 64, P(tab), 8, True, False, c, P(m), cnt), PTR),
        (mult(full, 64, P(tab), 0, True, False, c, P(m), cnt), ARG),
        (mult(full, 65, P(tab), 8, True, False, c, P(m), cnt), ARG),
        (lsum(full, 64, P(tab), P(m), 8, P(one), None, c, P(out), None), PTR),
        (lsum(full, 64, P(tab), P(m), 0, P(one), None, c, P(out), None), ARG),
        (lsum(full, 65, P(tab), P(m), 8, P(one), None, c, P(out), None), ARG),
    ]
    for k, (got, want) in enumerate(cases):
        assert got == want, k
    assert not m.any() and not out.any() and not one.any() and not any(cnt)
