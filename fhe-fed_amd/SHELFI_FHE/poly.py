"""Host helpers of EvalPoly: the plan of device.eval_poly as a dict, and a polynomial fit.

Nothing here touches a device."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check

MAX_DEGREE = 31


def plan(moduli: Sequence[int], scale_bits: int, coeffs: Sequence[float], towers: int, scale: float,
         combine_scale: Optional[float] = None) -> dict:
    """shelfi_poly_plan (include/shelfi.h states every rule): the Paterson-Stockmeyer plan of p(x) = sum_i coeffs[i]
    x^i, 1 <= degree <= 31, for an input ciphertext of `towers` towers at `scale` on the chain `moduli` with
    `scale_bits` scaling bits.  Returns the schedule (`powers`: one dict per power, every factor before its product,
    with n, a, b, towers, scale), the combine level and scale, the result's towers and scale after `rescales`
    rescales, the constants' scales [G][4] and their residues `table` [G][4][combine_towers] (uint64)."""
    a = np.ascontiguousarray(np.asarray(coeffs, np.float64).reshape(-1))
    if a.size < 2 or a.size > MAX_DEGREE + 1:
        raise ValueError("EvalPoly takes degrees 1..%d (2..%d coefficients)" % (MAX_DEGREE, MAX_DEGREE + 1))
    q = np.ascontiguousarray(np.asarray([int(v) for v in moduli], np.uint64))
    s = _lib.PolySchedule()
    check(_lib.load().shelfi_poly_plan(len(q), q.ctypes.data_as(_lib.u64p), int(scale_bits), a.ctypes.data_as(_lib.f64p),
                                       a.size - 1, int(towers), float(scale),
                                       0.0 if combine_scale is None else float(combine_scale), C.byref(s)), "poly_plan")
    tc, G = s.combine_towers, s.giants
    table = np.ctypeslib.as_array(s.table).copy()
    return {
        "degree": s.degree, "giants": G, "babies": s.babies, "rescales": s.rescales,
        "powers": [{"n": s.power_n[i], "a": s.power_a[i], "b": s.power_b[i], "towers": s.power_towers[i],
                    "scale": s.power_scale[i]} for i in range(s.num_powers)],
        "combine_towers": tc, "combine_scale": s.combine_scale,
        "result_towers": s.result_towers, "result_scale": s.result_scale,
        "const_scale": np.ctypeslib.as_array(s.const_scale).copy()[:G],
        "table": np.ascontiguousarray(table[:G, :, :tc]),
    }


def fit(f: Callable, lo: float, hi: float, degree: int) -> np.ndarray:
    """Monomial coefficients a_0 .. a_degree of the polynomial that interpolates f at the degree + 1 Chebyshev nodes
    of [lo, hi] (near-minimax for a smooth f), for device.eval_poly.  f takes and returns a numpy array.

    Conditioning: the monomial basis is badly conditioned away from [-1, 1].  On a wide or off-centre interval the
    coefficients grow like (2 / (hi - lo))^degree times binomial factors and cancel against each other, in float64
    here and again under encryption, where every power carries its own noise.  Normalise the INPUT first -- have the
    ciphertext hold t = (x - mid) / half, e.g. by scaling the values before encryption or with mult_plain /
    add_plain -- and fit f(mid + half t) on [-1, 1]."""
    if not 1 <= int(degree) <= MAX_DEGREE:
        raise ValueError("EvalPoly takes degrees 1..%d" % MAX_DEGREE)
    lo, hi, d = float(lo), float(hi), int(degree)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("fit needs a finite interval lo < hi")
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    t = np.cos(np.pi * (2 * np.arange(d + 1) + 1) / (2 * (d + 1)))
    y = np.asarray(f(mid + half * t), np.float64)
    c = np.polynomial.chebyshev.chebfit(t, y, d)        # d + 1 nodes, degree d: the interpolant
    pt = np.polynomial.Polynomial(np.polynomial.chebyshev.cheb2poly(c))
    px = pt(np.polynomial.Polynomial([-mid / half, 1 / half]))   # t = (x - mid) / half
    a = np.zeros(d + 1)
    a[:len(px.coef)] = px.coef
    return a
