"""Built ciphertexts with a planted decryption error, and the oracle's verdict on each: the inputs of
tests/test_gpu_decode_flood.py (CPU only; tests/test_flood_cases.py holds this module to closed forms).

As in tests/test_gpu_decode_edge.py a ciphertext is built, not encrypted: c1 = 0 and c0 = the per-tower
forward NTT of chosen integer coefficients c, so c0 + c1 s is exactly c under any key.  Slot i's coefficient
pair is (re_i, im_i) = (c[i gap], c[N/2 + i gap]) / scale.  PALISADE's Decode estimates the decryption error
from the anti-symmetric part u of the pairs (oracle or_decode_stats): u_0 = 2 im_0, u_{S/2} = re + im of slot
S/2, and for 0 < i < S/2 the two components re_i + im_{S-i} and im_i + re_{S-i}; sigma = 0.5 stddev(u) with
the mean taken out and S - 1 in the denominator.  A message with real slot values contributes nothing to u.

A case is a symmetric message part (O.encode_coeffs of a real vector; P0z and P4c: none) plus planted integers:

  P0, P0z     nothing: sigma sits on the floor sqrt(N)/8; P0z's variance is exactly 0 (log2(0), no failure)
  P1          im_0 = A: slot 0 counts 2 im_0, sigma = 2A / (2 sqrt S)
  P2a, P2b    slot S/2: re = A / re = A, im = -A: counts re + im; P2b is the floor (a sign error gives 2A)
  P3@i        re_i = A: one component, sigma = A / (2 sqrt S) for every i (not 0, not S/2)
  P3x@i       re_i = A, im_{S-i} = -A: the partner is S - i and the component cancels: the floor
  P4          every component of u is mu + e (im_0 = mu/2, re_{S/2} = mu, re_i = mu + e_i otherwise; e uniform
              in +-mu/16, mu = 2^30): the mean is taken out; mu / stddev(e) ~ 28
  P4c, P4c@j  every component exactly mu_j = 2^20 + 8198 j (j = 0 .. 7; no message, whose cancellation would leave
              half a unit of rounding in each component): the true variance is 0, and a one-pass
              variance sum u^2 - (sum u)^2 / S is a rounding residue of either sign, at most ~20 x 2^-53 S mu^2, i.e.
              a sigma_p below 0.03 -- far under the floor when positive, and a NaN (which fails the p - 5 check)
              when negative unless it is clamped to 0
  P5a, P5b    i.i.d. Gaussian error whose estimated sigma_p is 2^(p-6) / 2^(p-4): passes / fails the p - 5 check
  P6          Gaussian error, estimated sigma_p ~ 3000 (well above the floor): carries sqrt(M + 1)

A = 2^30 times the case's `amp`.  build() raises amp by 1.2 until log2(stddev_p sqrt(2S)) is at least 0.05
from a half-integer, so that logError never rests on a rounding tie.  The floor cases have nothing to scale;
their argument is 2^k sqrt(N 2S)/8 sqrt(M+1), which at M + 1 = 2^40 is a power of two unless log2 N + log2 S
is even, and then 2^j fl(sqrt 2): fl(sqrt 2) > sqrt 2, so every log2 within one ulp returns j + 0.5 or more
and rint gives j + 1 on the host and on the device alike (the 32-slot, 2^11 shape)."""
import math
from dataclasses import dataclass

import numpy as np

import oracle as O

A0 = 1 << 30
MU = 1 << 30
M_BIG = 2.0 ** 40 - 1
PAIRS_PER_WG = 1024  # decode_stats_kernel's kFloodPairsPerWg
FLOOR_CASES = ("P0", "P0z", "P2b", "P3x", "P4c")


def bitrev(i: int, bits: int) -> int:
    r = 0
    for _ in range(bits):
        r = (r << 1) | (i & 1)
        i >>= 1
    return r


def stats_pair(m: int):
    """FFT-input positions (P, partner) of decode_stats_kernel's pair m (0 <= m < S/2 - 1), from the mapping in
    the kernel's comment: m + 1 = 2^(h-1) + o, P = 2^h + o, partner 2^(h+1) - 1 - o."""
    hb = (m + 1).bit_length() - 1  # h - 1
    o = m + 1 - (1 << hb)
    return (2 << hb) + o, (4 << hb) - 1 - o


def pair_slot(m: int, S: int) -> int:
    """The slot at position P of pair m (slot i sits at FFT-input position bitrev(i))."""
    return bitrev(stats_pair(m)[0], S.bit_length() - 1)


def edge_pairs(S: int):
    """First and last pair of every decode_stats_kernel workgroup (G = S/2048 of them, 1024 pairs each; the last
    pair of all is m = S/2 - 2, which is also m1 - 1 under m1 = min(S/2 - 1, ...))."""
    half = S // 2
    G = max(1, half // PAIRS_PER_WG)
    ms = []
    for g in range(G):
        for m in (g * PAIRS_PER_WG, min(g * PAIRS_PER_WG + PAIRS_PER_WG - 1, half - 2)):
            if m not in ms:
                ms.append(m)
    return ms


def p3_slots(S: int):
    """The slots P3 / P3x visit: 1 and S/2 - 1, and from 4096 slots on the workgroup edges of the statistics."""
    out = [i for i in (1, S // 2 - 1) if 0 < i < S and i != S // 2]
    if S >= 4096:
        out += [pair_slot(m, S) for m in edge_pairs(S)]
    return list(dict.fromkeys(out))


def case_ids(S: int):
    """Every planted case of a shape with S >= 4 slots, in a fixed order (P5b, which raises, last)."""
    ids = ["P0", "P0z", "P1", "P2a", "P2b"]
    ids += ["P3@%d" % i for i in p3_slots(S)] + ["P3x@%d" % i for i in p3_slots(S)]
    return ids + ["P4", "P4c"] + ["P4c@%d" % j for j in range(1, 8)] + ["P5a", "P6", "P5b"]


@dataclass
class Shape:
    N: int
    S: int
    q: np.ndarray
    psi: np.ndarray
    delta: float
    p_bits: int = 52

    @classmethod
    def of(cls, info: dict, towers: int = 0) -> "Shape":
        """From CKKS.info(); towers: the first `towers` of the chain (a lower level), 0 = all."""
        t = towers or info["num_towers"]
        return cls(info["ring_dim"], info["batch"], np.array(info["moduli"][:t], np.uint64),
                   np.array(info["roots"][:t], np.uint64), info["delta"], info["scale_bits"])

    @classmethod
    def generate(cls, batch: int, ring: int, depth: int = 1, scale_bits: int = 52, first_mod_bits: int = 60):
        q, psi = O.params_generate(ring, depth + 1, scale_bits, first_mod_bits)
        return cls(ring, batch, q, psi, float(int(q[-1])), scale_bits)

    @property
    def gap(self) -> int:
        return self.N // (2 * self.S)

    @property
    def floor_p(self) -> float:
        return 0.125 * math.sqrt(self.N)


@dataclass
class Verdict:
    case: str
    amp: float
    res: np.ndarray  # [2][T][N] residues, c1 = 0
    sd: float        # the oracle's stddev at scale 2^p
    le: int          # logError
    fail: bool       # PALISADE's Decode would throw
    exact: np.ndarray = None  # the noise-free decode of the first n slots
    fl: np.ndarray = None     # the flooded decode at (seed, g)

    def nsd(self, sh: Shape) -> float:
        return self.sd / 2.0 ** sh.p_bits

    def bound(self, sh: Shape) -> float:
        """B of the tolerance: the noise a slot carries per unit normal."""
        return self.nsd(sh) * (math.sqrt(sh.S) if sh.S >= 64 else 2.0 * sh.S)


def _message(sh: Shape, tag: int) -> np.ndarray:
    x = np.random.default_rng(1000 + tag).uniform(-1, 1, sh.S)
    return O.encode_coeffs(x, sh.N, sh.S, sh.delta).astype(np.int64)


def _gauss_ints(sh: Shape, sigma_p_est: float, amp: float, tag: int):
    """(re, im) error integers whose *estimated* sigma_p is about sigma_p_est: a component of u is the sum of
    two coefficients' errors, and sigma = stddev(u) / 2, so each coefficient carries sqrt(2) sigma_p_est."""
    sd = math.sqrt(2.0) * sigma_p_est * amp * sh.delta / 2.0 ** sh.p_bits
    z = np.random.default_rng(2000 + tag).standard_normal((2, sh.S))
    return np.rint(z * sd).astype(np.int64)


def coeffs(sh: Shape, case: str, amp: float = 1.0, tag: int = 0) -> np.ndarray:
    """The case's N integer coefficients (int64)."""
    S, gap, h = sh.S, sh.gap, sh.S // 2
    name, _, at = case.partition("@")
    c = np.zeros(sh.N, np.int64) if name in ("P0z", "P4c") else _message(sh, tag)
    re = c[:S * gap:gap]        # views: re[i] = c[i gap]
    im = c[sh.N // 2::gap]      # im[i] = c[N/2 + i gap]
    assert re.shape == (S,) and im.shape == (S,)
    A = int(A0 * amp)
    if name in ("P0", "P0z"):
        pass
    elif name == "P1":
        im[0] += A
    elif name == "P2a":
        re[h] += A
    elif name == "P2b":
        re[h] += A
        im[h] -= A
    elif name in ("P3", "P3x"):
        i = int(at)
        assert 0 < i < S and i != h
        re[i] += A
        if name == "P3x":
            im[S - i] -= A
    elif name in ("P4", "P4c"):
        mu = 2 * (int(MU * amp) // 2) if name == "P4" else 2 * ((1 << 19) + 4099 * int(at or 0))
        e = np.zeros(S, np.int64)
        if name == "P4":
            e = np.random.default_rng(3000 + tag).integers(-(mu // 16), mu // 16 + 1, S)
        others = np.ones(S, bool)
        others[[0, h]] = False
        im[0] += mu // 2
        re[h] += mu
        re[others] += mu + e[others]
    elif name in ("P5a", "P5b", "P6"):
        target = {"P5a": 2.0 ** (sh.p_bits - 6), "P5b": 2.0 ** (sh.p_bits - 4), "P6": 3000.0}[name]
        e = _gauss_ints(sh, target, amp, tag)
        re += e[0]
        im += e[1]
    else:
        raise ValueError(case)
    return c


def residues(sh: Shape, c: np.ndarray) -> np.ndarray:
    """(c0, c1) = (NTT(c) per tower, 0): [2][T][N] uint64."""
    res = np.zeros((2, len(sh.q), sh.N), np.uint64)
    for t, (qt, pt) in enumerate(zip(sh.q, sh.psi)):
        res[0, t] = O.ntt_fwd(np.mod(c, np.int64(int(qt))).astype(np.uint64), int(qt), int(pt))
    return res


def _no_key(sh: Shape) -> np.ndarray:
    return np.zeros((len(sh.q), sh.N), np.uint64)  # c1 = 0: any key decrypts to c


def stats(sh: Shape, res: np.ndarray, m_factor: float):
    re, im = O.decrypt_coeffs(res, _no_key(sh), sh.q, sh.psi, sh.S, sh.delta)
    return O.decode_stats(re, im, sh.N, sh.p_bits, m_factor)


def half_integer_distance(sh: Shape, sd: float) -> float:
    t = math.log2(sd * math.sqrt(2.0 * sh.S)) - 0.5
    return abs(t - round(t))


def build(sh: Shape, case: str, m_factor: float = M_BIG, seed: int = 0, g: int = 0, n: int = None,
          tag: int = 0, amp: float = 1.0) -> Verdict:
    """The case's residues and the oracle's verdicts; with a seed also the flooded decode of stream index g."""
    name = case.partition("@")[0]
    for _ in range(8):
        res = residues(sh, coeffs(sh, case, amp, tag))
        sd, le, fail = stats(sh, res, m_factor)
        if name in FLOOR_CASES or half_integer_distance(sh, sd) >= 0.05:
            break
        amp *= 1.2
    else:
        raise AssertionError("no amplitude of %s keeps logError off a rounding tie" % case)
    if name in ("P5a", "P5b"):  # the verdict must not rest on the estimate's own spread
        s0 = stats(sh, res, 0.0)[0]  # M = 0: stddev_p = max(sigma_p, floor)
        d = math.log2(s0) - (sh.p_bits - 5)
        assert (d <= -0.5 and not fail) if name == "P5a" else (d >= 0.5 and fail), (case, d, fail)
    v = Verdict(case, amp, res, sd, le, fail)
    n = sh.S if n is None else n
    v.exact = O.decrypt(res, _no_key(sh), sh.q, sh.psi, sh.S, sh.delta, n)
    if seed:
        v.fl, le2, fail2 = O.decrypt_flood(res, _no_key(sh), sh.q, sh.psi, sh.S, sh.delta, n, seed=seed, g=g,
                                           p_bits=sh.p_bits, m_factor=m_factor)
        assert (le2, fail2) == (le, fail)
    return v
