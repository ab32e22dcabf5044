"""CPU-only: the Fr scan entries are declared in the header, exported by the built library and listed
in the binding's EXPORTED with their argument lists; the geometry entry, which does no device work,
answers on a machine without a GPU."""
import subprocess

import test_abi as A

NAMES = {"mbls_fr_prefix_product": 8, "mbls_fr_poly_divide_linear": 6, "mbls_fr_scan_geometry": 2}

built = A.built  # the module fixture that builds the library when it is missing


def test_header_declares_scans():
    fns = A.header_functions()
    for name in NAMES:
        assert name in fns, name


def test_library_exports_scans(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for name in NAMES:
        assert name in exported, name


def test_binding_lists_scans(built):
    amd = A._amd()
    for name in NAMES:
        assert name in amd.EXPORTED, name
    L = amd.lib()
    for name, nargs in NAMES.items():  # the binding gave each an argument list
        assert getattr(L, name).argtypes is not None, name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert callable(amd.prefix_product) and callable(amd.poly_divide_linear) and callable(amd.scan_geometry)


def test_geometry_is_consistent(built):
    amd = A._amd()
    g1 = amd.scan_geometry(1)
    K, T = g1["K"], g1["tile"]
    assert K >= 1 and T % K == 0 and g1["groups"] == 1 and g1["span"] == T
    for n in (T, T + 1, 5 * T + 3, 1 << 22, (1 << 26) - 1, 1 << 26):
        g = amd.scan_geometry(n)
        assert (g["K"], g["tile"]) == (K, T)
        assert g["span"] % T == 0 and 1 <= g["groups"] <= 1024
        assert (g["groups"] - 1) * g["span"] < n <= g["groups"] * g["span"]  # the spans just cover n
    for bad in (0, (1 << 26) + 1):
        try:
            amd.scan_geometry(bad)
        except amd.IcicleError as e:
            assert e.code == amd.INVALID_ARGUMENT
        else:
            raise AssertionError(bad)
