"""CPU-only: the G1 EC-NTT entry is declared in the header, exported by the built library and
listed in the binding's EXPORTED."""
import subprocess

import test_abi as A

NAMES = ["mbls_g1_ecntt"]

built = A.built  # the module fixture that builds the library when it is missing


def test_header_declares_ecntt():
    fns = A.header_functions()
    for name in NAMES:
        assert name in fns, name


def test_library_exports_ecntt(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for name in NAMES:
        assert name in exported, name


def test_binding_lists_ecntt(built):
    amd = A._amd()
    for name in NAMES:
        assert name in amd.EXPORTED, name
    L = amd.lib()
    for name in NAMES:  # the binding gave each an argument list
        assert getattr(L, name).argtypes is not None, name
    assert callable(amd.ecntt)
