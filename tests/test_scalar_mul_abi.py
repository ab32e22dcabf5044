"""CPU-only: the batch scalar multiplication entries are declared in the header, exported by the
built library and listed in the binding's EXPORTED."""
import subprocess

import test_abi as A

NAMES = ["bls12_381_g1_scalar_mul", "bls12_381_g1_scalar_mul_glv", "bls12_381_g2_scalar_mul",
         "mbls_g1_scalar_mul", "mbls_g2_scalar_mul"]

built = A.built  # the module fixture that builds the library when it is missing


def test_header_declares_scalar_mul():
    fns = A.header_functions()
    for name in NAMES:
        assert name in fns, name


def test_library_exports_scalar_mul(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for name in NAMES:
        assert name in exported, name


def test_binding_lists_scalar_mul(built):
    amd = A._amd()
    for name in NAMES:
        assert name in amd.EXPORTED, name
    L = amd.lib()
    for name in NAMES:  # the binding gave each an argument list
        assert getattr(L, name).argtypes is not None, name
    assert callable(amd.scalar_mul)
