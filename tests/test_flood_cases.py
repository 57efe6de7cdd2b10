"""tests/flood_cases.py held to closed forms (CPU): the planted cases decide what their table says they
decide, through the oracle alone.  With one non-zero component a of u, the mean is a / S and the variance
a^2 (1 - 1/S) / (S - 1) = a^2 / S, so sigma = |a| / (2 sqrt S) whichever component it is."""
import math

import numpy as np
import pytest

import flood_cases as F
import oracle as O

SHAPES = {"32/2^11": (32, 2048, 1), "64/2^11": (64, 2048, 1), "4096/2^13": (4096, 8192, 1),
          "8192/2^14": (8192, 16384, 2)}
_shapes = {}


def _shape(name):
    if name not in _shapes:
        _shapes[name] = F.Shape.generate(*SHAPES[name])
    return _shapes[name]


def _sigma_p(sh, v):
    """The estimate itself (above the floor): stddev_p at M = 0."""
    return F.stats(sh, v.res, 0.0)[0]


@pytest.mark.parametrize("name", list(SHAPES))
def test_single_component_sigma_is_a_over_two_sqrt_s(name):
    sh = _shape(name)
    unit = 2.0 ** sh.p_bits / sh.delta  # an integer coefficient in 2^p units
    cases = ["P1", "P2a"] + ["P3@%d" % i for i in F.p3_slots(sh.S)]
    for case in cases:
        v = F.build(sh, case)
        A = int(F.A0 * v.amp)
        a = 2 * A if case == "P1" else A  # slot 0 counts 2 im_0
        want = a * unit / (2.0 * math.sqrt(sh.S))
        assert want > 100 * sh.floor_p
        # the message's rounding (half a unit per coefficient) is all that separates the two
        assert _sigma_p(sh, v) == pytest.approx(want, rel=1e-6), case
        assert v.sd == pytest.approx(math.sqrt(F.M_BIG + 1) * want, rel=1e-6) and not v.fail
        assert v.le == int(np.rint(math.log2(v.sd * math.sqrt(2 * sh.S))))
        assert F.half_integer_distance(sh, v.sd) >= 0.05


def test_tie_avoidance_scales_the_amplitude():
    """A0 at 64 slots and M + 1 = 2^40 is 2^20 2^30 / 16 sqrt(128) = 2^49.5 (delta ~ 2^52): a tie, so build()
    must have moved it."""
    sh = _shape("64/2^11")
    v = F.build(sh, "P3@1")
    assert v.amp > 1.0
    res = F.residues(sh, F.coeffs(sh, "P3@1", 1.0))
    assert F.half_integer_distance(sh, F.stats(sh, res, F.M_BIG)[0]) < 0.05


@pytest.mark.parametrize("name", list(SHAPES))
def test_cancelling_cases_sit_on_the_floor(name):
    sh = _shape(name)
    cases = ["P0", "P0z", "P2b", "P4c"] + ["P4c@%d" % j for j in range(1, 8)] + ["P3x@%d" % i for i in F.p3_slots(sh.S)]
    assert set(cases) <= set(F.case_ids(sh.S))
    for case in cases:
        for M in (0.0, 1.0, F.M_BIG):
            v = F.build(sh, case, M)
            assert v.sd == pytest.approx(math.sqrt(M + 1) * sh.floor_p, rel=1e-15), (case, M)
            assert not v.fail
            assert v.le == int(np.rint(math.log2(math.sqrt(M + 1) * sh.floor_p * math.sqrt(2 * sh.S))))
    # P0z: the variance is exactly 0 -- log2(0) = -inf passes the p - 5 check
    re, im = O.decrypt_coeffs(F.build(sh, "P0z").res, np.zeros((len(sh.q), sh.N), np.uint64), sh.q, sh.psi, sh.S,
                              sh.delta)
    assert not re.any() and not im.any()
    # and a wrong partner or sign would not: P3x's planted pair alone is far above the floor
    i = F.p3_slots(sh.S)[0]
    assert _sigma_p(sh, F.build(sh, "P3@%d" % i)) > 100 * sh.floor_p


@pytest.mark.parametrize("name", list(SHAPES))
def test_mean_is_taken_out(name):
    """P4: every component is mu + e.  Two-pass sigma = stddev(e) / 2 ~ mu / (32 sqrt 3); without the mean it
    would be ~ mu / 2."""
    sh = _shape(name)
    v = F.build(sh, "P4")
    unit = 2.0 ** sh.p_bits / sh.delta
    mu = F.MU * v.amp * unit
    got = _sigma_p(sh, v)
    assert got == pytest.approx(mu / (32 * math.sqrt(3.0)), rel=4.0 / math.sqrt(sh.S))
    assert got < mu / 20 and not v.fail


@pytest.mark.parametrize("name", list(SHAPES))
def test_precision_threshold_verdicts(name):
    sh = _shape(name)
    a, b = F.build(sh, "P5a"), F.build(sh, "P5b")  # build() asserts the half-bit margins
    assert not a.fail and b.fail
    assert math.log2(_sigma_p(sh, a)) == pytest.approx(sh.p_bits - 6, abs=0.5)
    assert math.log2(_sigma_p(sh, b)) == pytest.approx(sh.p_bits - 4, abs=0.5)


@pytest.mark.parametrize("name", list(SHAPES))
def test_m_factor_scales_by_sqrt_m_plus_one(name):
    sh = _shape(name)
    v0 = F.build(sh, "P6", 0.0)
    base = _sigma_p(sh, v0) / v0.amp  # the estimate at amp = 1
    assert base == pytest.approx(3000.0, rel=4.0 / math.sqrt(sh.S)) and base > 10 * sh.floor_p
    for M in (0.0, 1.0, 3.0, F.M_BIG):
        v = F.build(sh, "P6", M)
        assert v.sd == pytest.approx(math.sqrt(M + 1) * _sigma_p(sh, v), rel=1e-15)
        assert _sigma_p(sh, v) == pytest.approx(base * v.amp, rel=1e-3)


@pytest.mark.parametrize("S", [64, 4096, 8192, 16384, 65536])
def test_stats_pairs_against_brute_force(S):
    """decode_stats_kernel's pair m -> positions (P, partner) against the definition: slot i sits at position
    bitrev(i), and its partner is slot S - i.  Pairs 0 .. S/2 - 2 cover every slot but 0 and S/2 once."""
    logS = S.bit_length() - 1
    pos = {i: F.bitrev(i, logS) for i in range(S)}  # slot -> position
    slot = {p: i for i, p in pos.items()}
    assert pos[0] == 0 and pos[S // 2] == 1
    seen = set()
    for m in range(S // 2 - 1):
        P, Q = F.stats_pair(m)
        i, j = slot[P], slot[Q]
        assert i + j == S and i not in (0, S // 2)
        assert not ({i, j} & seen)
        seen |= {i, j}
        assert F.pair_slot(m, S) == i
    assert seen == set(range(1, S)) - {S // 2}
    G = max(1, S // 2 // F.PAIRS_PER_WG)
    edges = F.edge_pairs(S)
    assert edges[-1] == S // 2 - 2 and edges[0] == 0
    if S >= 4096:
        want = sorted({1024 * g for g in range(G)} | {min(1024 * g + 1023, S // 2 - 2) for g in range(G)})
        assert sorted(edges) == want
        got = F.p3_slots(S)
        assert got[:2] == [1, S // 2 - 1] and set(got[2:]) | {1, S // 2 - 1} == {1, S // 2 - 1} | {
            slot[F.stats_pair(m)[0]] for m in want}
    else:
        assert F.p3_slots(S) == [1, S // 2 - 1]


def test_flooded_verdict_is_the_exact_decode_plus_scaled_normals():
    """build()'s flooded reference at 64 slots and more: exact + nsd sqrt(S) z with the oracle's output-domain
    normals of stream index g -- the quantity the tolerance's B scales."""
    sh = _shape("64/2^11")
    v = F.build(sh, "P6", F.M_BIG, seed=77, g=5)
    z = O.flood_out_normals(77, 5, sh.S)
    assert v.bound(sh) > 1e-7  # far above the subtraction's own rounding (values below 1: 2^-52)
    assert np.abs((v.fl - v.exact) - v.bound(sh) * z).max() <= 4 * 2.0 ** -52
    assert not np.array_equal(v.fl, F.build(sh, "P6", F.M_BIG, seed=77, g=6).fl)
