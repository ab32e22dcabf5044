"""CPU-only model of the membership criteria mbls_g*_check_points runs: on members, random curve
points, a torsion point of every prime of each cofactor (the 448-bit prime factor of h2 included) and
member + torsion sums, the endomorphism criteria

    G1: phi(P) + P == [z^2] P          G2: psi(P) == [z] P

agree with the definition [r]P == O taken by an unreduced double-and-add.  This pins the choice of
beta (oracle/pyref.py GLV_BETA) and of psi's sign that the kernel shares."""
import pytest

import subgroup_cases as S
from helpers import pyref as pr


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_members_pass_both(group):
    gen = S.ops(group)[3]
    mul = pr.g1_mul if group == "g1" else pr.g2_mul
    for k in (1, 2, 12345, pr.R - 1):
        p = mul(k, gen)
        assert S.in_subgroup(group, p), k
        assert S.criterion(group, p), k


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_random_curve_points_agree(group):
    on_curve = S.ops(group)[2]
    for p in S.random_curve_points(group, 3):
        assert on_curve(p)
        assert S.criterion(group, p) == S.in_subgroup(group, p)
        assert not S.in_subgroup(group, p)  # a random point of E(Fp) / E'(Fp2) carries a cofactor part


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_torsion_points_fail_both(group):
    on_curve, factors = S.ops(group)[2], S.ops(group)[5]
    tors = S.torsion_points(group)
    assert len(tors) == len(factors)
    for (l, _), t in zip(factors, tors):
        assert on_curve(t) and t is not None
        assert S.mul_raw(group, l, t) is None, l  # order exactly l (l is prime, t != O)
        assert not S.in_subgroup(group, t), l
        assert not S.criterion(group, t), l


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_member_plus_torsion_fails_both(group):
    on_curve, factors = S.ops(group)[2], S.ops(group)[5]
    for (l, _), p in zip(factors, S.member_plus_torsion(group)):
        assert on_curve(p)
        assert not S.in_subgroup(group, p), l
        assert not S.criterion(group, p), l


def test_g1_order_three_points():
    """(0, 2) and (0, p - 2): x = 0 but not the identity; doubling gives the negative"""
    a, b = (0, 2), (0, pr.P - 2)
    assert pr.g1_on_curve(a) and pr.g1_add(a, a) == b and pr.g1_add(pr.g1_add(a, a), a) is None
    for p in (a, b):
        assert not S.in_subgroup("g1", p) and not S.criterion("g1", p)


def test_chain_constants():
    assert S.Z2 == 0xac45a4010001a4020000000100000000 == pr.GLV_LAMBDA + 1
    assert S.Z2.bit_length() == 128 and bin(S.Z2).count("1") == 17
    assert S.Z_ABS.bit_length() == 64 and bin(S.Z_ABS).count("1") == 6
    assert S.H1 * pr.R == pr.P + 1 - (-S.Z_ABS + 1)  # #E(Fp) = p + 1 - t, t = z + 1


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_status_table_by_definition(group):
    """the fixed rows of the table have the statuses the issue names; every listed non-member is
    on the curve and outside the subgroup"""
    st = [S.expected(group, c) for c in S.status_table(group)]
    assert st[:8] == [S.OK, S.OK, S.OK, S.IDENTITY, S.NONCANONICAL, S.NONCANONICAL, S.OFF_CURVE, S.OFF_CURVE]
    assert st[8:] == [S.OFF_SUBGROUP] * len(S.non_members(group))
    assert len(set(S.non_members(group))) == len(S.non_members(group)) <= 100
