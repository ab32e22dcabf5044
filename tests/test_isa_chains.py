"""What the compiler makes of the inline-asm arithmetic chains (no GPU: cross-compiles to assembly).

tests/diag/chains_probe.hip holds one small kernel per primitive.  Each is compiled for gfx950 and
counted with tools/isa_chains.py:
  * v_mad_u64_u32 equals the formula's count (a dropped or duplicated term would show);
  * the packed radix-2^28 products are emitted in exactly the statements mbls_madchain.hpp's rule
    gives -- per column ceil(terms / 14), terms = [the previous column's closing step] + products +
    reduction terms -- 40 for mul where the split form had 117, and carry no more wait states
    (`s_nop`) than the form gave when it was chosen: 22 for mul (split: 99), 11 for sqr, 40 for mul2,
    57 for mul4;
  * the forms left as they were (the radix-2^29 Fr product, the row arithmetic) keep the pad counts
    recorded when the Fq form was chosen (profiles/r08/README.md), as a record of what a later change
    to them starts from."""
import os
import sys

import pytest

import helpers as H

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
import isa_chains  # noqa: E402

PROBE = os.path.join(H.ROOT, "tests", "diag", "chains_probe.hip")
NL, MAXP = 14, 14


def packed_statements(products_per_term):
    """statements of one radix-2^28 product whose column k holds products_per_term(k) product terms"""
    total = 0
    for k in range(2 * NL - 1):
        lo = max(0, k - (NL - 1))
        reduction = min(k, NL) - lo
        tail = 1 if 0 < k <= NL else 0
        total += -(-(tail + products_per_term(k) + reduction) // MAXP)
    return total


def col_n(k):
    return min(k, NL - 1) - max(0, k - (NL - 1)) + 1


def sqr_n(k):
    return (k + 1) // 2 - max(0, k - (NL - 1)) + (1 if k % 2 == 0 else 0)


@pytest.fixture(scope="module")
def counts():
    if not isa_chains.hipcc():
        pytest.skip("hipcc not available")
    inc = [os.path.join(H.ROOT, "midnight-bls12-381-cuda_amd", "csrc"), os.path.join(H.ROOT, "include")]
    return isa_chains.count_kernels(isa_chains.compile_asm(PROBE, inc))


def test_statement_rule():
    assert packed_statements(col_n) == 40
    assert sum(col_n(k) for k in range(27)) == 196 and sum(sqr_n(k) for k in range(27)) == 105


# primitive: (v_mad_u64_u32 of the formula, products per column for the packed forms, s_nop bound: the
# count the form gives, as recorded when it was chosen -- the split form gave 99 / 92 / 147 / 255)
PACKED = {
    "probe_r28_mul": (196 + 196, col_n, 22),
    "probe_r28_sqr": (105 + 196, sqr_n, 11),
    "probe_r28_mul2": (2 * 196 + 196, lambda k: 2 * col_n(k), 40),
    "probe_r28_mul4": (4 * 196 + 196, lambda k: 4 * col_n(k), 57),
}


@pytest.mark.parametrize("name", sorted(PACKED))
def test_packed_products(counts, name):
    mads, per_col, pads = PACKED[name]
    c = counts[name]
    print(name, dict(c))
    assert c["v_mad_u64_u32"] == mads
    assert c["asm"] == packed_statements(per_col)
    assert c["s_nop"] <= pads
    assert c["ScratchSize"] == 0


# primitive: (v_mad_u64_u32, asm statements, s_nop bound) of the forms left as they were
KEPT = {
    "probe_r29_mul_words": (81 + 72, 54, 34),  # 9 x 9 products, 72 reduction terms (r_0 = 1 is an addition)
    "probe_row_mul": (48, 41, 36),             # 12 rounds of m, v, w and the a_0 (-p^-1) b_i addend
    "probe_row_add": (0, 5, 7),
    "probe_row_sub": (0, 5, 13),
}


@pytest.mark.parametrize("name", sorted(KEPT))
def test_kept_forms(counts, name):
    mads, statements, pads = KEPT[name]
    c = counts[name]
    print(name, dict(c))
    assert c["v_mad_u64_u32"] == mads
    assert c["asm"] == statements
    assert c["s_nop"] <= pads
    assert c["ScratchSize"] == 0
