"""CPU-only: the model of the compressed encoding (tests/serde_model.py) against the published
generator encodings and against itself -- decode(encode(P)) == P on members, their negatives and
the special points, and the status of every malformed kind."""
import pytest

import serde_model as M
import subgroup_cases as S
from helpers import pyref as pr

GROUPS = ["g1", "g2"]


def test_generators_encode_as_published():
    assert M.encode("g1", pr.G1).hex() == M.G1_HEX
    assert M.encode("g2", pr.G2).hex() == M.G2_HEX
    assert M.decode("g1", bytes.fromhex(M.G1_HEX)) == (M.OK, pr.G1)
    assert M.decode("g2", bytes.fromhex(M.G2_HEX)) == (M.OK, pr.G2)


@pytest.mark.parametrize("group", GROUPS)
def test_infinity(group):
    rec = M.encode(group, None)
    assert rec == b"\xc0" + bytes(M.SIZE[group] - 1)
    assert M.decode(group, rec) == (M.IDENTITY, None)


@pytest.mark.parametrize("group", GROUPS)
def test_round_trip_members_negatives_and_specials(group):
    neg, on_curve = S.ops(group)[1], S.ops(group)[2]
    special = M.g1_specials() if group == "g1" else M.g2_specials()
    for p in M.member_points(group) + special:
        assert on_curve(p)
        rec, nrec = M.encode(group, p), M.encode(group, neg(p))
        assert M.decode(group, rec) == (M.OK, p)
        assert M.decode(group, nrec) == (M.OK, neg(p))
        # the negative flips S and nothing else
        assert nrec == bytes([rec[0] ^ M.S_BIT]) + rec[1:]
        assert rec[0] & M.C_BIT and not rec[0] & M.I_BIT


def test_generator_and_its_negative_differ_in_sign():
    for group in GROUPS:
        gen, last = M.member_points(group)[:2]
        assert last == S.ops(group)[1](gen)
        assert M.y_is_larger(group, gen[1]) != M.y_is_larger(group, last[1])


def test_g1_specials_sit_on_the_boundary():
    pts = M.g1_specials()
    assert pts[:2] == ((0, 2), (0, pr.P - 2))
    assert not M.y_is_larger("g1", 2) and M.y_is_larger("g1", pr.P - 2)
    above, below = pts[2], pts[4]
    # equal in every 32-bit word but the lowest: the comparison is decided there
    assert above[1] > M.HALF >= below[1]
    assert above[1] >> 32 == below[1] >> 32 == M.HALF >> 32
    assert M.y_is_larger("g1", above[1]) and not M.y_is_larger("g1", below[1])


def test_g2_specials_walk_the_root():
    pts = M.g2_specials()
    real, imag = pts[0], pts[1]
    for x, _ in (real, imag):
        assert M.radicand("g2", x)[1] == 0 and x[1] != 0
    assert real[1][1] == 0 and real[1][0] != 0       # y = (s, 0): S decided on c0
    assert imag[1][0] == 0 and imag[1][1] != 0       # y = (0, t)
    assert [p[0] for p in pts[2:5]] == [(2, 0), (4, 0), (5, 0)]
    for p in pts:
        assert pr.g2_on_curve(p)


@pytest.mark.parametrize("group", GROUPS)
def test_malformed_statuses(group):
    cases = M.malformed(group)
    kinds = [s for _, s in cases]
    assert set(kinds) == {M.BAD_FLAGS, M.NONCANONICAL, M.NO_POINT}
    assert kinds.count(M.NO_POINT) == 6
    for rec, want in cases:
        assert M.decode(group, rec) == (want, None), rec.hex()
    # a clear C wins over everything after it, infinity over the canonical test
    x = M.no_point_xs(group)[0]
    assert M.decode(group, M.raw_record(group, x, 0))[0] == M.BAD_FLAGS
    big = (1 << 381) - 1
    assert M.decode(group, M.raw_record(group, big if group == "g1" else (big, big), 0))[0] == M.BAD_FLAGS


@pytest.mark.parametrize("group", GROUPS)
def test_no_point_stream(group):
    xs = M.no_point_xs(group)
    assert len(xs) == 3 and len(set(xs)) == 3
    for x in xs:
        assert S.curve_point(group, None, x=x) is None


@pytest.mark.parametrize("group", GROUPS)
def test_status_table_holds_every_kind(group):
    records, st, pts = M.status_table(group)
    assert len(records) == len(st) == len(pts)
    assert set(int(v) for v in st) == {M.OK, M.IDENTITY, M.NONCANONICAL, M.NO_POINT, M.BAD_FLAGS}
    assert all((p is not None) == (s == M.OK) for p, s in zip(pts, st))
    assert M.words(group, pts).shape == (len(records), 12 if group == "g1" else 24)
