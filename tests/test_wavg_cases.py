"""CPU checks of tests/wavg_cases.py: the parameter rows reach every packed width class, the
saturating inputs really sit at the accumulators' limits (derived from the Python-int model of the
kernels' limb sums, not measured on a GPU), and the C oracle agrees with a Python-int weighted
sum on them.  The GPU side is tests/test_gpu_wavg_limits.py."""
import numpy as np
import pytest

import arena_layout as AL
import oracle as O
import wavg_cases as WC

TWO64 = 1 << 64


def _chain(row):
    scale, first, depth = row
    q, _ = O.params_generate(WC.RING, depth + 1, scale, first)
    return q, float(int(q[-1]))  # Delta = q_{L-1} (what CKKS.info()["delta"] reports)


def test_param_rows_cover_every_class():
    by_class = {}
    for row in WC.PARAM_ROWS:
        scale, first, depth = row
        assert 10 <= scale <= 58 and scale <= first <= 60  # validate_params
        q, _ = _chain(row)
        assert AL.widths(q) == [WC.width(x) for x in q]
        for x, U in zip(q, AL.widths(q)):
            by_class.setdefault(U, set()).add(int(x).bit_length())
    assert sorted(by_class) == WC.ALL_CLASSES
    assert {58, 59, 60} <= by_class[60]
    assert min(by_class[56]) < 56
    assert (52, 60, 1) in WC.PARAM_ROWS and (52, 60, 3) in WC.PARAM_ROWS


@pytest.mark.parametrize("row", WC.PARAM_ROWS)
def test_saturating_weight_and_edges(row):
    """The float32 weight's limbs, recomputed as the library and the oracle compute W; the edge
    residues are canonical and hold both limbs' and the packed field's extremes."""
    q, delta = _chain(row)
    for t in range(len(q)):
        qt = int(q[t])
        w, w0, w1 = WC.saturating_weight(t, q, delta)
        assert w < 0 and float(np.float32(w)) == w
        W = int(float(np.float32(w)) * delta + 0.5)
        assert W == O.weight_to_int(w, delta) and -(1 << 63) <= W < 0
        assert (w0, w1) == WC.limbs(W % qt) == WC.limbs(O.lib.or_mod_signed(W, qt))
        x0, x1 = WC.limbs(WC.xmax(qt))
        assert x0 - 64 < w0 <= x0 and w1 == x1 == max((qt >> 30) - 1, 0)
        assert x0 == min(qt - 1, WC.M30)
        e = WC.edge_residues(qt)
        assert all(0 <= x < qt for x in e) and len(set(e)) == len(e)
        assert {0, 1, qt - 1, qt - 2, WC.xmax(qt)} <= set(e)
        U = WC.width(qt)
        if U % 4 == 1:
            assert {(1 << (U - 1)) - 1, 1 << (U - 1)} <= set(e)  # field all ones; flag bit only
            assert ((1 << (U - 1)) | WC.M30) in e or ((1 << (U - 1)) | WC.M30) >= qt
        if qt > (1 << 30):
            assert {WC.M30, 1 << 30, (qt >> 30) << 30} <= set(e)


def peak_fractions(row):
    """{(tower, bits, scheme, accumulator): peak / 2^64} at the all-xmax positions of build_case with
    C = the group size and every learner at the saturating weight."""
    q, delta = _chain(row)
    out = {}
    for t in range(len(q)):
        qt = int(q[t])
        for scheme in ("three", "four"):
            G = WC.group_size(qt, scheme)
            case = WC.build_case(q, delta, G, t, 1)
            Ws = [WC.weight_int(w, delta) for w in case.w_sat]
            per_pos = []
            for j in case.sat:
                xs = [int(ct[0, 1, t, j]) for ct in case.cts]
                assert xs == [WC.xmax(qt)] * G
                per_pos.append(WC.accumulators(xs, Ws, qt, scheme))
            assert all(a == per_pos[0] for a in per_pos)
            for name, v in per_pos[0].items():
                out[(t, qt.bit_length(), scheme, name)] = v
    return q, out


@pytest.mark.parametrize("row", WC.PARAM_ROWS)
def test_accumulators_sit_at_their_limits(row):
    """At the all-xmax positions with C = G learners every limb sum is < 2^64, and
      * each saturable sum (S0 at G = 16, Sm at a 60-bit tower with G = 8; s00 everywhere and
        s01, s10, s11 at a 60-bit tower) has peak (G + 1) >= G 2^64: one more learner of that size in
        the group wraps it, so a group widened by one fails the GPU test;
      * no overflow can be staged in the others (Sm below 60 bits, S1 everywhere, S0 at G = 8, the
        mixed and high sums of the four-sum kernels below 60 bits): their limb ranges bound them far
        under 2^64.  There the peak is at least half of that analytic bound, so the inputs are still
        the largest available.  Sums over a high limb are exempt when q_t >> 30 < 4 (towers of at
        most 32 bits): xmax puts the low limb first, its high limb is (q_t >> 30) - 1 in 0..2 and the
        sums stay below 2^37."""
    q, peaks = peak_fractions(row)
    for (t, bits, scheme, name), v in sorted(peaks.items()):
        qt = int(q[t])
        G = WC.group_size(qt, scheme)
        bound = WC.accumulator_bounds(qt, scheme)[name]
        print("%s tower %d (%d bits) %-5s G=%2d %-3s peak/2^64 = %.9f" % (row, t, bits, scheme, G, name, v / TWO64))
        assert v < TWO64 and v <= bound
        if name in WC.saturable(qt, scheme):
            assert v * (G + 1) >= G * TWO64, (t, scheme, name)
        elif name in ("S0", "s00") or (qt >> 30) >= 4:
            assert bound < TWO64 and 2 * v >= bound, (t, scheme, name)
        else:
            assert bound < 1 << 37
    # the 60-bit tower's saturable sets are exercised by the rows that have one
    if int(q[0]).bit_length() == 60:
        assert WC.saturable(int(q[0]), "three") == ("Sm",) and len(WC.saturable(int(q[0]), "four")) == 4


@pytest.mark.parametrize("row", WC.PARAM_ROWS)
def test_oracle_wavg_equals_python_ints(row):
    """oracle.wavg (C, 128-bit products) == sum_c W_c x_c mod q_t in Python ints on the planted and
    sampled positions, for the saturating and the mixed weight vectors."""
    q, delta = _chain(row)
    for t in range(len(q)):
        case = WC.build_case(q, delta, 17, t, 2)
        for w in (case.w_sat, case.w_mix):
            ref = O.wavg(case.cts, w, q, delta)
            Ws = [WC.weight_int(x, delta) for x in w]
            exact = WC.wavg_exact(case.cts, Ws, q, case.positions)
            assert [int(ref[pos]) for pos in case.positions] == exact
        assert len(case.positions) >= 2 * 2 * len(case.sat) + 64


@pytest.mark.parametrize("row,cls", [((30, 33, 2), 33), ((37, 40, 2), 37), ((44, 49, 2), 44),
                                     ((44, 49, 2), 49), ((48, 56, 2), 56)])
def test_pack_roundtrip_new_classes(row, cls):
    """arena_layout's pack / unpack round-trips a two-learner case that holds the edge residues, for
    the width classes the earlier suite never ran."""
    q, delta = _chain(row)
    assert cls in AL.widths(q)
    case = WC.build_case(q, delta, 2, AL.widths(q).index(cls), 1)
    words = AL.pack_arena(case.cts, q, WC.RING)
    assert words.size == 2 * 2 * WC.RING * sum(AL.widths(q)) // 32
    back = AL.unpack_arena(words, 2, 1, len(q), WC.RING, q)
    for a, b in zip(case.cts, back):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("row", WC.PARAM_ROWS)
def test_pack_one_equals_pack_arena(row):
    """The vectorised one-learner packer the GPU tests build packed blobs with == the lane-by-lane
    restatement of the layout, on a saturating case of every row (K = 2)."""
    q, delta = _chain(row)
    case = WC.build_case(q, delta, 1, len(q) - 1, 2)
    assert np.array_equal(AL.pack_one(case.cts[0], q, WC.RING), AL.pack_arena(case.cts, q, WC.RING))
