"""shelfi_poly_plan without a device: the host-only plan of EvalPoly equals tests/poly_ref.py's
restatement in Python ints, Fractions and the stated double operations, field for field, for every degree 1..31 on
a 52 / 60-bit chain of 7 towers ("A"), one of 12 ("C") and a 30 / 45-bit one of 4 ("G") -- where both refuse, both
must refuse; and every refusal include/shelfi.h lists leaves the output struct untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import poly_ref as PR
from SHELFI_FHE import _lib
from SHELFI_FHE import poly as P

# id: (ring, towers, scale bits, first modulus bits) -- tests/test_gpu_gram.py's chains of the same names
CHAINS = {"A": (1 << 12, 7, 52, 60), "C": (1 << 12, 12, 52, 60), "G": (1 << 12, 4, 30, 45)}


@functools.lru_cache(maxsize=None)
def _q(cid):
    N, L, sb, fb = CHAINS[cid]
    return [int(v) for v in O.params_generate(N, L, sb, fb)[0]]


def _both(cid, coeffs, l, s1, Sc=None):
    """(library plan, restated plan), or (None, None) when BOTH refuse; one refusing alone fails."""
    q, sb = _q(cid), CHAINS[cid][2]
    try:
        ref = PR.plan(q, sb, coeffs, l, s1, Sc)
    except ValueError:
        ref = None
    try:
        got = P.plan(q, sb, coeffs, l, s1, Sc)
    except ValueError:
        got = None
    assert (got is None) == (ref is None), (cid, len(coeffs) - 1, l)
    return got, ref


def _same(got, ref):
    for key in ("degree", "giants", "babies", "rescales", "combine_towers", "result_towers"):
        assert got[key] == ref[key], key
    for key in ("combine_scale", "result_scale"):  # doubles, bit for bit
        assert np.float64(got[key]).tobytes() == np.float64(ref[key]).tobytes(), key
    assert len(got["powers"]) == len(ref["powers"])
    for a, b in zip(got["powers"], ref["powers"]):
        assert (a["n"], a["a"], a["b"], a["towers"]) == (b["n"], b["a"], b["b"], b["towers"])
        assert np.float64(a["scale"]).tobytes() == np.float64(b["scale"]).tobytes(), a["n"]
    assert got["const_scale"].tobytes() == ref["const_scale"].tobytes()
    assert got["table"].dtype == np.uint64 and np.array_equal(got["table"], ref["table"])


def _coeffs(d, kind, rng):
    a = rng.normal(0, 1, d + 1)
    if kind == "mixed":  # negative, zero and tiny coefficients among ordinary ones
        a[rng.integers(0, d + 1)] = 0.0
        a[rng.integers(0, d + 1)] = -0.0
        a[rng.integers(0, d + 1)] = 1e-30        # rounds to W = 0 at every scale in reach
        a[rng.integers(0, d + 1)] = -5e-324      # the smallest subnormal
        a[d] = -abs(a[d]) - 0.5
    elif kind == "large":
        a *= 1e6
    return a


@pytest.mark.parametrize("cid", ["A", "C", "G"])
@pytest.mark.parametrize("d", range(1, 32))
def test_plan_equals_the_restatement(cid, d):
    q, L = _q(cid), CHAINS[cid][1]
    rng = np.random.default_rng([d, L])
    s1 = float(q[L - 1])
    accepted = 0
    for kind in ("plain", "mixed", "large"):
        for l in (L, L - 1):
            got, ref = _both(cid, _coeffs(d, kind, rng), l, s1)
            if got is not None:
                _same(got, ref)
                accepted += 1
    # a non-default combine scale, no power of two; and an input scale that is not a modulus
    got, ref = _both(cid, _coeffs(d, "mixed", rng), L, s1 * 1.0000003, 3.0 * 2.0 ** (2 * CHAINS[cid][2] - 3))
    if got is not None:
        _same(got, ref)
        assert got["combine_scale"] == 3.0 * 2.0 ** (2 * CHAINS[cid][2] - 3)
    if cid == "C":  # 12 towers hold every degree
        assert accepted == 6


def test_depth_table():
    """ceil(log2(highest power)) + r levels: 3 at d = 3, 4 at d = 7, 6 at d = 15 (a plain power basis: 3 / 4 / 5)."""
    q = _q("C")
    for d, levels in ((1, 1), (2, 2), (3, 3), (4, 4), (7, 4), (8, 5), (11, 5), (12, 6), (15, 6), (16, 6), (19, 6),
                      (20, 7), (31, 7)):
        pl = P.plan(q, 52, [1.0] * (d + 1), 12, float(q[11]))
        assert 12 - pl["result_towers"] == levels, d
        assert pl["rescales"] == (1 if d <= 3 else 2) and pl["giants"] == (d + 4) // 4
        for p in pl["powers"]:
            assert 12 - p["towers"] == (p["n"] - 1).bit_length(), p  # ceil(log2 n)


def test_schedule_is_the_stated_one():
    pl = P.plan(_q("C"), 52, [1.0] * 32, 12, float(_q("C")[11]))
    assert [(p["n"], p["a"], p["b"]) for p in pl["powers"]] == [
        (1, 0, 0), (2, 1, 1), (3, 2, 1), (4, 2, 2), (8, 4, 4), (12, 8, 4), (16, 8, 8), (20, 16, 4), (24, 16, 8),
        (28, 16, 12)]
    assert pl["combine_scale"] == 2.0 ** 156 and pl["combine_towers"] == 7
    assert P.plan(_q("C"), 52, [1.0] * 4, 12, float(_q("C")[11]))["combine_scale"] == 2.0 ** 104


def test_a_product_exactly_on_a_half_rounds_away_from_zero():
    q = _q("A")
    s1 = float(q[6])
    # term (0, 0) is encoded at c = S_c: the default 2^104, then 3 * 2^100 (a product with a three-bit mantissa)
    for Sc, a, w in ((None, 1.5 * 2.0 ** -104, 2), (None, -1.5 * 2.0 ** -104, -2), (None, 2.5 * 2.0 ** -104, 3),
                     (3.0 * 2.0 ** 100, 2.0 ** -101, 2), (3.0 * 2.0 ** 100, -(2.0 ** -101), -2),
                     (None, np.nextafter(1.5, 0) * 2.0 ** -104, 1), (None, 0.5 * 2.0 ** -104, 1),
                     (None, np.nextafter(0.5, 0) * 2.0 ** -104, 0)):
        got, ref = _both("A", [a, 1.0, 0.0, 1.0], 7, s1, Sc)
        _same(got, ref)
        assert ref["W"][0, 0] == w
        assert [int(v) for v in got["table"][0, 0]] == [w % m for m in q[:got["combine_towers"]]]


def _raw(q, sb, coeffs, d, l, s1, Sc, out):
    qa = np.array(q, np.uint64)
    ca = None if coeffs is None else np.array(coeffs, np.float64)
    return _lib.load().shelfi_poly_plan(len(q), qa.ctypes.data_as(_lib.u64p), sb,
                                        None if ca is None else ca.ctypes.data_as(_lib.f64p), d, l, s1, Sc,
                                        None if out is None else C.byref(out))


def test_refusals_write_nothing():
    q = _q("A")
    s1 = float(q[6])
    out = _lib.PolySchedule()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    before = bytes(out)
    ok = [1.0, -2.0, 0.5, 0.25]
    refused = [
        lambda: _raw(q, 52, [1.0], 0, 7, s1, 0.0, out),                      # d = 0
        lambda: _raw(q, 52, [1.0] * 33, 32, 7, s1, 0.0, out),                # d = 32
        lambda: _raw(q, 52, [1.0, float("nan"), 0.5, 0.25], 3, 7, s1, 0.0, out),   # non-finite coefficients
        lambda: _raw(q, 52, [1.0, 2.0, float("inf"), 0.25], 3, 7, s1, 0.0, out),
        lambda: _raw(q, 52, [float("-inf"), 2.0, 0.5, 0.25], 3, 7, s1, 0.0, out),
        lambda: _raw(q, 52, ok, 3, 3, s1, 0.0, out),                         # t_c - r = 1 - 1 < 1
        lambda: _raw(q, 52, ok, 3, 2, s1, 0.0, out),                         # a power below one tower
        lambda: _raw(q, 52, [1.0] * 8, 7, 4, s1, 0.0, out),                  # t_c - r = 2 - 2
        lambda: _raw(q, 52, [1.0] * 21, 20, 7, s1, 0.0, out),                # P_20 needs 5 levels and r = 2
        lambda: _raw(q, 52, [1e300, 1.0, 0.5, 0.25], 3, 7, s1, 0.0, out),    # |W| >= Q / 2
        lambda: _raw(q, 52, [1.0, 1.0, 0.5, -1e70], 3, 7, s1, 0.0, out),
        lambda: _raw(q, 52, ok, 3, 7, s1, 2.0 ** 400, out),                  # ... through the combine scale
        lambda: _raw(q, 52, ok, 3, 0, s1, 0.0, out),                         # towers outside 1..L
        lambda: _raw(q, 52, ok, 3, 8, s1, 0.0, out),
        lambda: _raw(q, 52, ok, 3, 7, 0.0, 0.0, out),                        # scales
        lambda: _raw(q, 52, ok, 3, 7, float("inf"), 0.0, out),
        lambda: _raw(q, 52, ok, 3, 7, s1, -1.0, out),
        lambda: _raw(q, 52, ok, 3, 7, s1, float("nan"), out),
        lambda: _raw(q, 52, None, 3, 7, s1, 0.0, out),                       # NULL pointers
        lambda: _raw(q, 52, ok, 3, 7, s1, 0.0, None),
    ]
    for i, call in enumerate(refused):
        assert call() == _lib.SHELFI_ERR_ARG, i
        assert bytes(out) == before, i
    # near the edge on a real chain (G, t_c = 2, c = 2^60): the nearest doubles either side of Q / 2
    g = _q("G")
    Q = g[0] * g[1]
    for w, good in (((Q - 1) // 2, True), ((Q + 1) // 2, False)):
        a = w / 2.0 ** 60
        if int(a * 2.0 ** 60) != w:  # not representable: the nearest double on the right side of the edge
            a = float(np.nextafter(a, 0 if good else np.inf))
        got, ref = _both("G", [a, 1.0, 0.0, 1.0], 4, float(g[3]))
        assert (got is not None) == good
    assert _raw(q, 52, ok, 3, 7, s1, 0.0, out) == _lib.SHELFI_OK and out.result_towers == 4
    for v in ([1.0], [1.0] * 33):
        with pytest.raises(ValueError):
            P.plan(q, 52, v, 7, s1)


def _edge(q, a, Sc):
    """(accepted by the library, accepted by the restatement) for p(x) = a + x on the synthetic chain q at
    s_1 = 1 and combine scale Sc: term (0, 0) is W = round(a Sc) against Q = prod q."""
    out = _lib.PolySchedule()
    rc = _raw(q, 30, [a, 1.0], 1, len(q), 1.0, Sc, out)
    assert rc in (_lib.SHELFI_OK, _lib.SHELFI_ERR_ARG)
    try:
        ref = PR.plan(q, 30, [a, 1.0], len(q), 1.0, Sc)
    except ValueError:
        ref = None
    if rc == _lib.SHELFI_OK:
        assert ref is not None and out.combine_towers == len(q)
        for t in range(len(q)):
            assert out.table[0][0][t] == int(ref["table"][0, 0, t])
    return rc == _lib.SHELFI_OK, ref is not None


def test_the_edge_of_half_the_modulus_exactly():
    """2 |W| against Q at Q - 1, Q + 1 and Q itself, on synthetic chains handed straight to shelfi_poly_plan (it takes
    moduli, prime or not), every value an exact double.  Q odd: W = (Q - 1) / 2 is taken and (Q + 1) / 2 refused, in
    both signs (the branch that shifts the mantissa product right); Q = 3 * 2^140: W = Q / 2 is refused and the double below it taken (the branch that shifts it left)."""
    for q in ([7, 11], [33554467, 33554473], [2 ** 20 + 7, 2 ** 20 + 13, 2 ** 10 + 1]):
        Q = int(np.prod([int(v) for v in q], dtype=object))
        assert Q % 2 == 1 and Q < 2 ** 53
        for sign in (1.0, -1.0):
            assert _edge(q, sign * float((Q - 1) // 2), 1.0) == (True, True)
            assert _edge(q, sign * float((Q + 1) // 2), 1.0) == (False, False)
            assert _edge(q, sign * float((Q - 1) // 2) / 4.0, 4.0) == (True, True)     # the same W from a fraction
            assert _edge(q, sign * float((Q + 1) // 2) / 4.0, 4.0) == (False, False)
    q = [2 ** 50, 2 ** 50, 3 * 2 ** 40]  # Q = 3 * 2^140
    half = 3.0 * 2.0 ** 79               # times c = 2^60: W = 3 * 2^139 = Q / 2
    for sign in (1.0, -1.0):
        assert _edge(q, sign * half, 2.0 ** 60) == (False, False)
        assert _edge(q, sign * float(np.nextafter(half, 0)), 2.0 ** 60) == (True, True)
        assert _edge(q, sign * float(np.nextafter(half, np.inf)), 2.0 ** 60) == (False, False)
