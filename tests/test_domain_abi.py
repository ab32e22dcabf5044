"""CPU-only: the extended-coset transform entries are declared in the header, exported by the built
library and listed in the binding's EXPORTED with their argument lists; the plan entry, which does
no device work, equals tests/domain_model.py's; and every argument error comes back with its code
before the first HIP call, so on a machine without a GPU too."""
import ctypes
import subprocess

import numpy as np
import pytest

import domain_model as D
import test_abi as A

NAMES = {"mbls_fr_coeff_to_extended": 6, "mbls_fr_extended_to_coeff": 8, "mbls_fr_domain_plan": 3}

built = A.built  # the module fixture that builds the library when it is missing


def test_header_declares_domain():
    fns = A.header_functions()
    for name in NAMES:
        assert name in fns, name


def test_library_exports_domain(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for name in NAMES:
        assert name in exported, name


def test_binding_lists_domain(built):
    amd = A._amd()
    L = amd.lib()
    for name, nargs in NAMES.items():
        assert name in amd.EXPORTED, name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == nargs, name
    assert callable(amd.coeff_to_extended) and callable(amd.extended_to_coeff) and callable(amd.domain_plan)


def _sizes(N):
    s = {1, 2, 3, N}
    for k in range(N.bit_length()):
        s |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    return sorted(v for v in s if 1 <= v <= N)


def test_plan_equals_the_model(built):
    """mbls_fr_domain_plan reports ntt.hip's one pass plan (pass_plan), which the plain NTT
    (ntt_device) runs as well as the domain transforms: this pins the plan of both to ntt_model.plan."""
    amd = A._amd()
    for K in range(13):
        for size in _sizes(1 << K):
            assert amd.domain_plan(size, 1 << K) == D.plan(size, 1 << K), (size, K)
    for K in (22, 26):
        for size in (1, 3, (1 << (K - 3)) - 1, 1 << (K - 3), 1 << (K - 2), (1 << (K - 2)) + 1, 1 << K):
            assert amd.domain_plan(size, 1 << K) == D.plan(size, 1 << K), (size, K)
    p = amd.domain_plan(1 << 20, 1 << 22)
    assert (p["passes"], p["E"], p["skipped"], p["rows"], p["fwd_scratch"]) == (3, 2, 2, 64, 0)


def test_plan_argument_errors(built):
    amd = A._amd()
    out = (ctypes.c_int32 * D.PLAN_WORDS)()
    L = amd.lib()
    assert L.mbls_fr_domain_plan(1, 1, None) == amd.INVALID_POINTER
    for size, N in ((0, 8), (9, 8), (-1, 8), (1, 0), (1, 6), (1, -8), (3, 3)):
        assert L.mbls_fr_domain_plan(size, N, out) == amd.INVALID_ARGUMENT, (size, N)


def _call_fwd(amd, coeffs, size, N, g, cfg, out):
    return amd.lib().mbls_fr_coeff_to_extended(coeffs, size, N, g, cfg, out)


def _call_inv(amd, evals, N, m, g, vinv, period, cfg, out):
    return amd.lib().mbls_fr_extended_to_coeff(evals, N, m, g, vinv, period, cfg, out)


def test_argument_errors_before_any_device_work(built):
    amd = A._amd()
    buf = np.zeros((16, 4), dtype=np.uint64)
    out = np.zeros((16, 4), dtype=np.uint64)
    p, q = amd._p(buf), amd._p(out)
    cfg = amd.ntt_config()
    c = ctypes.byref(cfg)
    one = amd._coset_arg(D.mont_words(1))
    zero = amd._coset_arg([0, 0, 0, 0])
    r_itself = amd._coset_arg([(D.R >> (64 * i)) & ((1 << 64) - 1) for i in range(4)])  # zero mod r
    PTR, ARG = amd.INVALID_POINTER, amd.INVALID_ARGUMENT
    # null pointers
    assert _call_fwd(amd, None, 4, 16, one, c, q) == PTR
    assert _call_fwd(amd, p, 4, 16, one, None, q) == PTR
    assert _call_fwd(amd, p, 4, 16, one, c, None) == PTR
    assert _call_inv(amd, None, 16, 4, one, None, 0, c, q) == PTR
    assert _call_inv(amd, p, 16, 4, one, None, 0, None, q) == PTR
    assert _call_inv(amd, p, 16, 4, one, None, 0, c, None) == PTR
    # sizes
    for size, N in ((0, 16), (17, 16), (-3, 16), (4, 12), (4, 0), (1, -16)):
        assert _call_fwd(amd, p, size, N, one, c, q) == ARG, (size, N)
        assert _call_inv(amd, p, N, size, one, None, 0, c, q) == ARG, (size, N)
    # the vanishing period, only with a table
    for period in (0, -1, 3, 32):
        assert _call_inv(amd, p, 16, 4, one, p, period, c, q) == ARG, period
    # a generator that is zero mod r
    for g in (zero, r_itself):
        assert _call_fwd(amd, p, 4, 16, g, c, q) == ARG
        assert _call_inv(amd, p, 16, 4, g, None, 0, c, q) == ARG
    # columns_batch and orderings other than NN
    bad = [amd.ntt_config(columns_batch=True)] + [amd.ntt_config(ordering=o) for o in range(1, 6)]
    for b in bad:
        assert _call_fwd(amd, p, 4, 16, one, ctypes.byref(b), q) == ARG
        assert _call_inv(amd, p, 16, 4, one, None, 0, ctypes.byref(b), q) == ARG
    # the binding raises them as IcicleError
    with pytest.raises(amd.IcicleError) as e:
        amd.coeff_to_extended(buf[:5], 4, out=out)
    assert e.value.code == ARG
    assert not out.any()
