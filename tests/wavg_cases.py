"""Inputs that drive the aggregation kernels (fhe-fed_amd/csrc/wavg.hip) to the limits of their
carry-free limb sums, and a Python-int model of those sums.  Test infrastructure shared by
tests/test_wavg_cases.py (CPU) and tests/test_gpu_wavg_limits.py (GPU); numpy only.

The kernels split a residue x < q_t and a weight W mod q_t into 30-bit limbs (x0, x1), (w0, w1) and
sum limb products over a group of learners without carries:
  scheme "four"  (wavg_kernel, wavg_packed_r3): s00 = sum x0 w0, s01 = sum x0 w1, s10 = sum x1 w0,
                 s11 = sum x1 w1 over groups of 16 learners;
  scheme "three" (wavg_packed): S0 = sum x0 w0, Sm = sum (x0 w1 + x1 w0), S1 = sum x1 w1 over groups
                 of 16 learners up to the 57-bit width class and of 8 in the 60-bit class.
Every sum must stay below 2^64.  The cases here make every learner of a group contribute the largest
term canonical inputs allow: the residue xmax(q_t) (both limbs at their largest) under a float32
weight whose integer W is -(q_t - xmax(q_t)) or a few units below it, so W mod q_t is xmax(q_t)
less a few units as well."""
import types

import numpy as np

M30 = (1 << 30) - 1
RING = 1024

# (scaleFactorBits, firstModBits, multDepth) at ring 1024 (two 512-residue rows per tower).  Tower
# bit lengths -> packed width classes (test_wavg_cases.py::test_param_rows_cover_every_class):
PARAM_ROWS = [
    (52, 60, 1),  # 60, 53                         the reference chain, depth 1
    (58, 60, 3),  # 60, 59, 58, 59 bits            all in class 60
    (52, 60, 3),  # 60, 53, 52, 53                 the reference chain, depth 3
    (55, 58, 2),  # 58, 55, 56 bits                classes 60, 56, 56
    (54, 57, 2),  # 57, 54, 55 bits                classes 57, 56, 56
    (48, 56, 2),  # 56, 48, 49
    (44, 49, 2),  # 49, 44, 45
    (36, 41, 2),  # 41, 36, 37
    (37, 40, 2),  # 40, 37, 38 bits                classes 40, 37, 40
    (30, 33, 2),  # 33, 30, 31 bits                classes 33, 32, 32
    (46, 48, 1),  # 48, 47 bits                    classes 48, 48
    (58, 59, 1),  # 59, 59 bits                    class 60; q_0 just under 2^59, the largest 59-bit tower
]
ALL_CLASSES = [32, 33, 36, 37, 40, 41, 44, 45, 48, 49, 52, 53, 56, 57, 60]

# the lanes and row halves that carry xmax in every learner (build_case)
SAT_LANES = (0, 31, 63)


def width(qt):
    """Packed width class U_t of one tower (dev_api.cpp arena_pack; arena_layout.widths)."""
    b = int(qt).bit_length()
    return 32 if b <= 32 else (b if b % 4 == 1 else (b + 3) // 4 * 4)


def group_size(qt, scheme):
    """Learners per carry-free group: 16, but 8 for wavg_packed in the 60-bit width class."""
    return 8 if scheme == "three" and width(qt) > 57 else 16


def xmax(qt):
    """The canonical residue with the largest low limb and, under that, the largest high limb."""
    qt = int(qt)
    if qt <= M30:
        return qt - 1
    return (((qt >> 30) - 1) << 30) | M30


def edge_residues(qt):
    """Canonical residues that load each limb and each boundary of the packed field."""
    qt = int(qt)
    U = width(qt)
    B = U & ~3
    out = [0, 1, qt - 1, qt - 2, M30, 1 << 30, xmax(qt), (qt >> 30) << 30, (1 << B) - 1]
    if U % 4 == 1:
        out += [1 << B, (1 << B) | M30]
    seen = []
    for x in out:
        if 0 <= x < qt and x not in seen:
            seen.append(x)
    return seen


def weight_int(w, delta):
    """W = (int64)((double)(float)w * Delta + 0.5): truncation toward zero (call_state.cpp)."""
    return int(float(np.float32(w)) * float(delta) + 0.5)


def limbs(v):
    return int(v) & M30, int(v) >> 30


def saturating_weight(t, q, delta):
    """A float32 w < 0 whose W mod q_t has both limbs at (or a few units under) their largest:
    W = -(m + e) with m = q_t - xmax(q_t) and the smallest e >= 0 a float32 reaches.  Deterministic:
    the float32 neighbours of -m / Delta are walked away from zero.  -> (w, w0, w1)."""
    qt = int(q[t])
    m = qt - xmax(qt)
    # W truncates toward zero, so W <= -m needs w Delta <= -(m + 1/2)
    w = np.float32(-(m + 0.5) / float(delta))
    # step toward zero until W > -m (too small in magnitude), then away until W <= -m
    for _ in range(8):
        if -weight_int(w, delta) < m:
            break
        w = np.nextafter(w, np.float32(0))
    for _ in range(64):
        if -weight_int(w, delta) >= m:
            break
        w = np.nextafter(w, np.float32(-np.inf))
    W = weight_int(w, delta)
    assert W <= -m and w < 0
    w0, w1 = limbs(W % qt)
    return float(w), w0, w1


def accumulators(xs, Ws, qt, scheme):
    """Exact value of every carry-free sum the kernels form at one residue position over one group
    of learners (xs: residues, Ws: integer weights, any sign; len <= group_size)."""
    qt = int(qt)
    assert len(xs) == len(Ws) <= group_size(qt, scheme)
    acc = dict.fromkeys(("s00", "s01", "s10", "s11") if scheme == "four" else ("S0", "Sm", "S1"), 0)
    for x, W in zip(xs, Ws):
        x0, x1 = limbs(x)
        w0, w1 = limbs(int(W) % qt)
        if scheme == "four":
            acc["s00"] += x0 * w0
            acc["s01"] += x0 * w1
            acc["s10"] += x1 * w0
            acc["s11"] += x1 * w1
        else:
            acc["S0"] += x0 * w0
            acc["Sm"] += x0 * w1 + x1 * w0
            acc["S1"] += x1 * w1
    return acc


def accumulator_bounds(qt, scheme):
    """Analytic per-group bound of each sum from the limb ranges of canonical inputs alone:
    x0, w0 <= min(q - 1, 2^30 - 1) and x1, w1 <= q >> 30."""
    qt = int(qt)
    G, lo, hi = group_size(qt, scheme), min(qt - 1, M30), qt >> 30
    if scheme == "four":
        return {"s00": G * lo * lo, "s01": G * lo * hi, "s10": G * hi * lo, "s11": G * hi * hi}
    return {"S0": G * lo * lo, "Sm": 2 * G * lo * hi, "S1": G * hi * hi}


def saturable(qt, scheme):
    """The sums whose group is sized by the 2^64 limit: one more learner of the largest size would
    wrap.  Everything else stays far below 2^64 by its limb ranges."""
    bits = int(qt).bit_length()
    if scheme == "four":
        return ("s00", "s01", "s10", "s11") if bits == 60 else ("s00",)
    if group_size(qt, scheme) == 16:
        return ("S0",)
    return ("Sm",) if bits == 60 else ()


def sat_positions(N=RING):
    """Coefficient indices of the lanes SAT_LANES' eight residues 2l + (j & 1) + 128 (j >> 1) in
    every 512-residue row of a polynomial."""
    return [ch * 512 + 2 * l + (j & 1) + 128 * (j >> 1)
            for ch in range(N // 512) for l in SAT_LANES for j in range(8)]


def wavg_exact(cts, Ws, q, positions):
    """sum_c W_c x_c mod q_t in Python ints at positions (k, p, t, j) -> list of ints."""
    out = []
    for (k, p, t, j) in positions:
        out.append(sum(int(W) * int(ct[k, p, t, j]) for ct, W in zip(cts, Ws)) % int(q[t]))
    return out


def build_case(q, delta, C, target_tower, K, N=RING, seed=0):
    """C learner batches [K][2][L][N] (uint64) that saturate tower `target_tower`:
      * xmax(q_t) in all learners at sat_positions() of the target tower (both polys, every k);
      * the other edge residues of every tower at other positions, rotated by learner;
      * uniform random canonical residues elsewhere.
    w_sat gives every learner saturating_weight(target_tower); w_mix is the same but, at C > 2,
    learner 1 has weight 0.0 and learner 2 a positive one.  positions: the planted ones plus 64
    random ones per tower, as (k, p, t, j)."""
    L = len(q)
    rng = np.random.default_rng(seed * 1000003 + C * 101 + target_tower * 7 + K)
    sat = sat_positions(N)
    free = [j for j in range(N) if j not in set(sat)]
    cts = []
    positions = set()
    for c in range(C):
        a = np.empty((K, 2, L, N), np.uint64)
        for t in range(L):
            qt = int(q[t])
            a[:, :, t, :] = rng.integers(0, qt, (K, 2, N), dtype=np.uint64)
            edges = edge_residues(qt)
            # edges spread over both row halves, every lane parity and j: stride 13 through `free`
            for i in range(3 * len(edges)):
                j = free[(5 + 13 * i) % len(free)]
                a[:, :, t, j] = edges[(i + c) % len(edges)]
                if c == 0:
                    positions.update((k, p, t, j) for k in range(K) for p in range(2))
        a[:, :, target_tower, sat] = xmax(int(q[target_tower]))
        cts.append(a)
    positions.update((k, p, target_tower, j) for k in range(K) for p in range(2) for j in sat)
    for t in range(L):
        for j in rng.integers(0, N, 64):
            positions.add((int(rng.integers(0, K)), int(rng.integers(0, 2)), t, int(j)))
    w, w0, w1 = saturating_weight(target_tower, q, delta)
    w_sat = [w] * C
    w_mix = list(w_sat)
    if C > 2:
        w_mix[1] = 0.0
        w_mix[2] = 0.75
    return types.SimpleNamespace(cts=cts, w_sat=w_sat, w_mix=w_mix, positions=sorted(positions), sat=sat,
                                 target=target_tower, w_limbs=(w0, w1), K=K, C=C)
