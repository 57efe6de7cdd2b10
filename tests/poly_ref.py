"""Reference for EvalPoly, built from Python integers, fractions.Fraction and the oracle only.

  plan          shelfi_poly_plan restated: the schedule, every power's towers and scale with the stated double
                operations, and the constants W = sign(a) floor(|a| c + 1/2) on the exact product as Fractions
  combine_sums  shelfi_dev_poly_combine's three sums as exact modular arithmetic on the residues
  combine_ref   ... plus ONE batched relinearization: O.eval_mult of (0, d2) by (0, 1), plus (d0, d1), as
                tests/wsum_ref.py does
  powers_ref    the powers along the schedule: O.eval_mult on the operands' prefixes and O.rescale
  eval_poly_ref plan -> powers -> combine -> rescales

Test infrastructure only; nothing here is imported by the product."""
import math
from fractions import Fraction

import numpy as np

import oracle as O
import rotation_ref as R

MAX_DEGREE, MAX_TOWERS = 31, 16


def _good(v):
    return math.isfinite(v) and v > 0.0


def round_product(a, c):
    """sign(a) floor(|a| c + 1/2) for the exact product of the doubles a and c."""
    w = math.floor(Fraction(abs(a)) * Fraction(c) + Fraction(1, 2))
    return -w if a < 0 else w


def schedule(d):
    """[(n, a, b)]: P_n = P_a P_b, every factor before its product; (1, 0, 0) is the input."""
    G = (d + 4) // 4
    s = [(1, 0, 0)]
    if d >= 2:
        s.append((2, 1, 1))
    if d >= 3:
        s.append((3, 2, 1))
    if G > 1:
        s.append((4, 2, 2))
    for g in range(2, G):
        h = 1
        while h * 2 < g:
            h *= 2
        s.append((4 * g, 4 * h, 4 * (g - h)))
    return s


def plan(q, p, coeffs, l, s1, Sc=None, equal_scale=False):
    """The dict SHELFI_FHE.poly.plan returns, or ValueError where shelfi_poly_plan refuses.  q: the chain's moduli,
    p: its scaling bits, l / s1: the input's towers and scale.  equal_scale: the constants as a hand composition
    would encode them, every power taken to sit at s1 (NOT what the library does: for the drift comparison)."""
    q = [int(v) for v in q]
    a = [float(v) for v in coeffs]
    d = len(a) - 1
    if not 1 <= len(q) <= MAX_TOWERS or not 1 <= d <= MAX_DEGREE or not all(math.isfinite(v) for v in a):
        raise ValueError("degree or coefficients")
    if not 1 <= l <= len(q) or not 1 <= p <= 60 or not _good(s1) or not (Sc is None or Sc == 0.0 or _good(Sc)):
        raise ValueError("towers or scales")
    if any(v < 2 or v >> 60 for v in q):
        raise ValueError("moduli")
    G, nb, r = (d + 4) // 4, min(d, 3), (2 if d > 3 else 1)
    tw, sc, powers = {1: l}, {1: float(s1)}, []
    for n, x, y in schedule(d):
        if n > 1:
            t = min(tw[x], tw[y])
            if t < 2:
                raise ValueError("levels")
            tw[n] = t - 1
            sc[n] = (sc[x] * sc[y]) / float(q[t - 1])
            if not _good(sc[n]):
                raise ValueError("scale range")
        powers.append({"n": n, "a": x, "b": y, "towers": tw[n], "scale": sc[n]})
    tc = min(tw.values())
    if tc - r < 1:
        raise ValueError("levels")
    S = float(Sc) if Sc else 2.0 ** ((3 if G > 1 else 2) * p)
    Q = math.prod(q[:tc])
    cs, table = np.zeros((G, 4)), np.zeros((G, 4, tc), np.uint64)
    W = {}
    for g in range(G):
        for j in range(4):
            if 4 * g + j > d:
                continue
            c = S
            if g:
                c = c / (sc[1] if equal_scale else sc[4 * g])
            if j:
                c = c / (sc[1] if equal_scale else sc[j])
            if not _good(c):
                raise ValueError("scale range")
            cs[g, j] = c
            w = round_product(a[4 * g + j], c) if a[4 * g + j] != 0.0 else 0
            if 2 * abs(w) >= Q:
                raise ValueError("constant too large")
            W[g, j] = w
            table[g, j] = [w % q[t] for t in range(tc)]
    rs = S
    for i in range(r):
        rs = rs / float(q[tc - 1 - i])
    return {"degree": d, "giants": G, "babies": nb, "rescales": r, "powers": powers, "combine_towers": tc,
            "combine_scale": S, "result_towers": tc - r, "result_scale": rs, "const_scale": cs, "table": table,
            "W": W}


def combine_sums(babies, giants, table, towers, q):
    """d [K][3][towers][N]: the three sums of shelfi_dev_poly_combine (include/shelfi.h), canonical.  babies /
    giants: lists of [K][2][>= towers][N] uint64 arrays; table [len(giants) + 1][4][towers]."""
    babies = [np.asarray(b, np.uint64) for b in babies]
    giants = [np.asarray(g, np.uint64) for g in giants]
    table = np.asarray(table, np.uint64)
    nb, ng = len(babies), len(giants)
    assert 1 <= nb <= 3 and ng <= 7 and table.shape == (ng + 1, 4, towers)
    K, _, _, N = babies[0].shape
    assert all(v.shape[0] == K and v.shape[2] >= towers and v.shape[3] == N for v in babies + giants)
    d = np.zeros((K, 3, towers, N), np.uint64)
    for t in range(towers):
        m = np.uint64(q[t])

        def inner(g, i):  # q_{g,i} [K][N]
            acc = np.full((K, N), table[g, 0, t] if i == 0 else 0, np.uint64)
            for j in range(nb):
                acc = (acc + R.mulmod(table[g, 1 + j, t], babies[j][:, i, t], m)) % m
            return acc

        d0, d1, d2 = inner(0, 0), inner(0, 1), np.zeros((K, N), np.uint64)
        for g in range(1, ng + 1):
            q0, q1 = inner(g, 0), inner(g, 1)
            G0, G1 = giants[g - 1][:, 0, t], giants[g - 1][:, 1, t]
            d0 = (d0 + R.mulmod(G0, q0, m)) % m
            d1 = (d1 + R.mulmod(G0, q1, m)) % m
            d1 = (d1 + R.mulmod(G1, q0, m)) % m
            d2 = (d2 + R.mulmod(G1, q1, m)) % m
        d[:, 0, t], d[:, 1, t], d[:, 2, t] = d0, d1, d2
    return d


def combine_ref(babies, giants, table, towers, evk, q, psi):
    """[K][2][towers][N]: (d0, d1) + KeySwitch(d2); without giants (d0, d1) alone (no key: evk may be None)."""
    d = combine_sums(babies, giants, table, towers, q)
    if not giants:
        return np.ascontiguousarray(d[:, :2])
    K, _, l, N = d.shape
    X, Y = np.zeros((K, 2, l, N), np.uint64), np.zeros((K, 2, l, N), np.uint64)
    X[:, 1] = d[:, 2]
    Y[:, 1] = 1  # the constant 1 in EVALUATION
    out = O.eval_mult(X, Y, evk, q, psi)
    ql = np.asarray(q[:l], np.uint64)[None, None, :, None]
    return (out + d[:, :2]) % ql


def powers_ref(x, pl, evk, q, psi):
    """{n: P_n} along the plan's schedule: EvalMult on the operands' prefixes at the lower one's towers, ModReduce."""
    have = {1: np.asarray(x, np.uint64)}
    for p in pl["powers"]:
        if p["n"] == 1:
            continue
        a, b = have[p["a"]], have[p["b"]]
        t = min(a.shape[2], b.shape[2])
        prod = O.eval_mult(np.ascontiguousarray(a[:, :, :t]), np.ascontiguousarray(b[:, :, :t]), evk, q, psi)
        have[p["n"]] = O.rescale(prod, q, psi)
        assert have[p["n"]].shape[2] == p["towers"]
    return have


def eval_poly_ref(x, coeffs, scale, p, evk, q, psi, Sc=None, equal_scale=False):
    """(ct [K][2][result towers][N], scale): device.eval_poly's whole pipeline."""
    x = np.asarray(x, np.uint64)
    pl = plan(q, p, coeffs, x.shape[2], scale, Sc, equal_scale)
    have = powers_ref(x, pl, evk, q, psi)
    babies = [have[j] for j in range(1, pl["babies"] + 1)]
    giants = [have[4 * g] for g in range(1, pl["giants"])]
    out = combine_ref(babies, giants, pl["table"], pl["combine_towers"], evk, q, psi)
    for _ in range(pl["rescales"]):
        out = O.rescale(out, q, psi)
    return out, pl["result_scale"]
