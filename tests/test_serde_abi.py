"""CPU-only: the point compression / decompression entries are declared in the header, exported by
the built library and listed in the binding's EXPORTED; the binding's decode status constants match
the header's enum."""
import re
import subprocess

import test_abi as A

NAMES = {"mbls_g1_decompress": 7, "mbls_g2_decompress": 7, "mbls_g1_compress": 5, "mbls_g2_compress": 5}

built = A.built  # the module fixture that builds the library when it is missing


def test_header_declares_serde():
    fns = A.header_functions()
    for name in NAMES:
        assert name in fns, name


def test_library_exports_serde(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for name in NAMES:
        assert name in exported, name


def test_binding_lists_serde(built):
    amd = A._amd()
    for name in NAMES:
        assert name in amd.EXPORTED, name
    L = amd.lib()
    for name, nargs in NAMES.items():  # the binding gave each an argument list
        assert getattr(L, name).argtypes is not None, name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert callable(amd.decompress_points) and callable(amd.compress_points)


def test_decode_constants_match_the_header():
    amd = A._amd()
    src = open(A.HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"MBLS_DECODE_(\w+) = (\d+)", src))
    assert enum == {"OK": amd.DECODE_OK, "IDENTITY": amd.DECODE_IDENTITY, "NONCANONICAL": amd.DECODE_NONCANONICAL,
                    "NO_POINT": amd.DECODE_NO_POINT, "BAD_FLAGS": amd.DECODE_BAD_FLAGS}
    assert [enum[k] for k in ("OK", "IDENTITY", "NONCANONICAL", "NO_POINT", "BAD_FLAGS")] == [0, 1, 2, 3, 5]
    # 0..3 line up with mbls_point_status, and 4 stays MBLS_POINT_OFF_SUBGROUP's alone
    assert (amd.DECODE_OK, amd.DECODE_IDENTITY, amd.DECODE_NONCANONICAL) == \
        (amd.POINT_OK, amd.POINT_IDENTITY, amd.POINT_NONCANONICAL)
    assert amd.DECODE_NO_POINT == amd.POINT_OFF_CURVE and amd.POINT_OFF_SUBGROUP not in enum.values()
