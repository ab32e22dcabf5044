"""CPU-only checks of the sort and lookup entries at the library boundary: the three names are
declared, exported and bound; mbls_fr_sort_plan is consistent across sizes; every documented argument
error comes back before any device work, so also on a machine without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import lookup_model as M

HEADER = os.path.join(H.ROOT, "include", "bls12_381_mi355x.h")
PKG = os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd")
LIB = os.path.join(PKG, "lib", "libbls12_381_mi355x.so")


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^eIcicleError\s+(\w+)\s*\(", src, flags=re.M))


NAMES = {"mbls_fr_sort": 6, "mbls_fr_lookup_permute": 8, "mbls_fr_sort_plan": 3}
MAX = 1 << 26


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
        assert name in fns, name
        assert name in exported, name
        assert name in amd.EXPORTED, name
        f = getattr(amd.lib(), name)
        assert len(f.argtypes) == nargs and f.restype is ctypes.c_int, name
    text = open(HEADER).read()
    assert "NOT constant time" in text and "standard-form integer value" in text


def test_sort_plan_is_consistent(amd):
    one = amd.sort_plan(1)
    bits, tile = one["bits"], one["tile"]
    assert bits == M.BITS and one["passes"] == 256 // bits
    assert tile == M.LIBRARY.wave * M.LIBRARY.waves * M.LIBRARY.rounds
    sizes = sorted({1, 2, tile - 1, tile, tile + 1, 2 * tile + 3, 1 << 16, (1 << 20) - 1, 1 << 20, (1 << 20) + 1,
                    tile * M.LIBRARY.max_groups, tile * M.LIBRARY.max_groups + 1, 1 << 22, (1 << 25) + 1, MAX - 1, MAX})
    last = None
    for n in sizes:
        p = amd.sort_plan(n)
        assert p["bits"] == bits and p["tile"] == tile and p["passes"] == one["passes"], n
        span, groups = M.sort_geom(n, M.LIBRARY)
        assert p["groups"] == groups, n
        assert 1 <= p["groups"] <= M.LIBRARY.max_groups, n
        per = -(-n // p["groups"])  # elements per workgroup, at the least
        tiles_per_group = -(-per // tile)
        assert p["groups"] * tiles_per_group * tile >= n, n            # the tiles cover size
        assert (p["groups"] - 1) * tiles_per_group * tile < n, n       # and no workgroup is empty
        assert p["sort_bytes"] >= 48 * n and p["lookup_bytes"] > 2 * 48 * n, n
        if last:
            assert p["sort_bytes"] >= last["sort_bytes"] and p["lookup_bytes"] >= last["lookup_bytes"], n
        last = p
    # a batch is one array of size * batch elements, plus the passes over the member number
    assert amd.sort_plan(tile + 1, 3)["groups"] == amd.sort_plan(3 * (tile + 1))["groups"]
    assert amd.sort_plan(5, 2)["passes"] == one["passes"] + 1
    assert amd.sort_plan(5, 256)["passes"] == one["passes"] + 1
    assert amd.sort_plan(5, 257)["passes"] == one["passes"] + 2
    assert amd.sort_plan(1, MAX)["sort_bytes"] == amd.sort_plan(MAX, 1)["sort_bytes"]


def test_sort_plan_rejects_sizes_out_of_range(amd):
    L = amd.lib()
    out = (ctypes.c_int64 * 6)()
    assert L.mbls_fr_sort_plan(0, 1, out) == amd.INVALID_ARGUMENT
    assert L.mbls_fr_sort_plan(MAX + 1, 1, out) == amd.INVALID_ARGUMENT
    assert L.mbls_fr_sort_plan((1 << 25) + 1, 2, out) == amd.INVALID_ARGUMENT
    assert L.mbls_fr_sort_plan(8, 0, out) == amd.INVALID_ARGUMENT
    assert L.mbls_fr_sort_plan(8, 1, None) == amd.INVALID_POINTER
    assert L.mbls_fr_sort_plan(MAX, 1, out) == amd.SUCCESS


def test_argument_errors_come_before_any_device_work(amd):
    L, P = amd.lib(), amd._p
    buf = np.zeros((8, 4), dtype=np.uint64)
    tab = np.zeros((8, 4), dtype=np.uint64)
    o1, o2 = np.zeros((8, 4), dtype=np.uint64), np.zeros((8, 4), dtype=np.uint64)
    perm = np.zeros(8, dtype=np.uint32)
    cnt = (ctypes.c_uint64 * 2)()
    c = ctypes.byref(amd.vec_config())
    c2 = ctypes.byref(amd.vec_config(batch_size=2))
    cols = ctypes.byref(amd.vec_config(batch_size=2, columns_batch=True))
    cases = [
        (L.mbls_fr_sort(None, 8, True, c, P(o1), P(perm)), amd.INVALID_POINTER),
        (L.mbls_fr_sort(P(buf), 8, True, None, P(o1), P(perm)), amd.INVALID_POINTER),
        (L.mbls_fr_sort(P(buf), 8, True, c, None, None), amd.INVALID_POINTER),
        (L.mbls_fr_sort(P(buf), 0, True, c, P(o1), None), amd.INVALID_ARGUMENT),
        (L.mbls_fr_sort(P(buf), MAX + 1, False, c, P(o1), None), amd.INVALID_ARGUMENT),
        (L.mbls_fr_sort(P(buf), (1 << 25) + 1, True, c2, None, P(perm)), amd.INVALID_ARGUMENT),
        (L.mbls_fr_sort(P(buf), 4, True, cols, P(o1), None), amd.API_NOT_IMPLEMENTED),
        (L.mbls_fr_lookup_permute(None, P(tab), 8, True, c, P(o1), P(o2), cnt), amd.INVALID_POINTER),
        (L.mbls_fr_lookup_permute(P(buf), None, 8, True, c, P(o1), P(o2), cnt), amd.INVALID_POINTER),
        (L.mbls_fr_lookup_permute(P(buf), P(tab), 8, True, None, P(o1), P(o2), cnt), amd.INVALID_POINTER),
        (L.mbls_fr_lookup_permute(P(buf), P(tab), 8, True, c, None, P(o2), cnt), amd.INVALID_POINTER),
        (L.mbls_fr_lookup_permute(P(buf), P(tab), 8, True, c, P(o1), None, None), amd.INVALID_POINTER),
        (L.mbls_fr_lookup_permute(P(buf), P(tab), 0, True, c, P(o1), P(o2), cnt), amd.INVALID_ARGUMENT),
        (L.mbls_fr_lookup_permute(P(buf), P(tab), MAX + 1, False, c, P(o1), P(o2), None), amd.INVALID_ARGUMENT),
        (L.mbls_fr_lookup_permute(P(buf), P(tab), (1 << 25) + 1, True, c2, P(o1), P(o2), cnt), amd.INVALID_ARGUMENT),
        (L.mbls_fr_lookup_permute(P(buf), P(tab), 4, True, cols, P(o1), P(o2), cnt), amd.API_NOT_IMPLEMENTED),
    ]
    for k, (got, want) in enumerate(cases):
        assert got == want, k
    assert not o1.any() and not o2.any() and not perm.any()
