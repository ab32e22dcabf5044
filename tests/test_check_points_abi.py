"""CPU-only: the point validation entries are declared in the header, exported by the built library
and listed in the binding's EXPORTED; the binding's status constants match the header's enum."""
import re
import subprocess

import test_abi as A

NAMES = ["mbls_g1_check_points", "mbls_g2_check_points"]

built = A.built  # the module fixture that builds the library when it is missing


def test_header_declares_check_points():
    fns = A.header_functions()
    for name in NAMES:
        assert name in fns, name


def test_library_exports_check_points(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for name in NAMES:
        assert name in exported, name


def test_binding_lists_check_points(built):
    amd = A._amd()
    for name in NAMES:
        assert name in amd.EXPORTED, name
    L = amd.lib()
    for name in NAMES:  # the binding gave each an argument list
        assert getattr(L, name).argtypes is not None, name
        assert len(getattr(L, name).argtypes) == 6, name
    assert callable(amd.check_points)


def test_status_constants_match_the_header():
    amd = A._amd()
    src = open(A.HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"MBLS_POINT_(\w+) = (\d+)", src))
    assert enum == {"OK": amd.POINT_OK, "IDENTITY": amd.POINT_IDENTITY, "NONCANONICAL": amd.POINT_NONCANONICAL,
                    "OFF_CURVE": amd.POINT_OFF_CURVE, "OFF_SUBGROUP": amd.POINT_OFF_SUBGROUP}
    assert [enum[k] for k in ("OK", "IDENTITY", "NONCANONICAL", "OFF_CURVE", "OFF_SUBGROUP")] == [0, 1, 2, 3, 4]
