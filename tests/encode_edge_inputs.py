"""Slot vectors that put encode's message coefficients m = round(FFTSpecialInv(x)_i / S * Delta) at the
edges of their range, for tests/test_encode_edge_inputs.py (CPU: every builder lands where it claims,
judged by the oracle) and tests/test_gpu_encode_edge.py (the HIP encrypt on every dispatch branch).

The ranges (fhe-fed_amd/csrc/encrypt.hip, "encode's large-value path"; oracle/ckks_oracle.c
or_encode_coeffs_ex):
  |m| <= 2^61                  the fast kernels; nothing is flagged
  2^61 < |m| <= 2^62 - 512     the call is redone (launch_encrypt_approx) with logApprox = 0
  |m| >= 2^62, logApprox = 0   FitToNativeVector's wrap at Max64BitValue() = 2^63 - 513 (glibc's log2 of
                               2^62 and of 2^62 + 1024 is 62.0, so ceil() leaves the exponent at 0)
  beyond                       logApprox = ceil(log2 |v|) - 62 > 0
  |v| = inf                    refused

Two shapes of x give exact control over the coefficients:
  * an impulse x[s] = a spreads over every coefficient position j as a cos(theta_{s,j}) / S (first half)
    and a sin(theta_{s,j}) / S (second half): with a = 0.99 * 2^61 * S / Delta every coefficient is
    0.99 * 2^61 * |cos| or |sin|: a dense band below the fast path's limit (two thirds above 2^60);
  * a constant vector c is the constant polynomial: coefficient 0 is fl(c * Delta), every other one is
    exactly 0 (the butterflies add equal values and subtract them to exact zeros), so one coefficient is
    placed to the ulp by stepping c with np.nextafter.
Everything is a function of a context's (N, S, Delta) alone."""
import collections
import functools

import numpy as np

import oracle as O

# name -> (batchSize, ringDim, multDepth, scaleFactorBits, firstModBits): the contexts whose encrypt
# takes a different chain of kernels (launch_encrypt), and two modulus classes
SHAPES = collections.OrderedDict([
    ("2^11/L2", (1024, 2048, 1, 52, 60)),
    ("2^12/L2", (2048, 4096, 1, 52, 60)),
    ("2^13/L2", (4096, 8192, 1, 52, 60)),
    ("2^14/L3", (8192, 16384, 2, 52, 60)),
    ("2^15/L4", (16384, 32768, 3, 52, 60)),
    ("2^15/gap2", (8192, 32768, 3, 52, 60)),
    ("2^15/gap4", (4096, 32768, 3, 52, 60)),
    ("2^16/L2", (32768, 65536, 1, 52, 60)),
    ("2^17/L2", (65536, 131072, 1, 52, 60)),
    ("30-bit", (4096, 8192, 1, 30, 40)),        # 40- / 31-bit towers: no one-step reduction
    ("41-bit/2^13", (4096, 8192, 1, 41, 45)),   # 45- / 42-bit towers
    ("41-bit/2^15", (16384, 32768, 3, 41, 45)),  # 45 / 42 / 41 / 42 bits: red_any's smallest class
])

Chain = collections.namedtuple("Chain", "N S L q psi delta")


@functools.lru_cache(maxsize=None)
def chain(name):
    """The oracle's parameters of a shape (the product's are checked against them on the GPU)."""
    batch, N, depth, sb, fb = SHAPES[name]
    q, psi = O.params_generate(N, depth + 1, sb, fb)
    return Chain(N, batch, depth + 1, q, psi, float(int(q[-1])))


def ckks_args(name, cryptodir):
    """Positional and keyword arguments of SHELFI_FHE.CKKS for a shape."""
    batch, N, depth, sb, fb = SHAPES[name]
    return ("ckks", batch, sb, cryptodir), dict(multDepth=depth, firstModBits=fb, ringDim=N)


# ------------------------------------------------------------------ dense_band ----
def impulse_slots(S, K):
    """Ciphertext k's impulse slot: S - 1, 0 and 1 first (a call of two has both ends), then spread over
    the vector, short of the last slots (a call's ragged last ciphertext keeps its impulse)."""
    fixed = [S - 1, 0, 1]
    return [fixed[k] if k < 3 else 2 + (5 + 37 * k) % (S - 18) for k in range(K)]


def dense_band(S, delta, K, seed=0, frac=0.99):
    """K ciphertexts' slots: uniform(-1, 1) with one impulse of +-frac 2^61 S / Delta each (the sign
    alternates): every nonzero-position coefficient is about frac 2^61 |cos| or |sin|, none above 2^61."""
    x = np.random.default_rng(1000 + seed).uniform(-1, 1, K * S)
    a = frac * 2.0 ** 61 * S / delta
    for k, s in enumerate(impulse_slots(S, K)):
        x[k * S + s] = a if k % 2 == 0 else -a
    return x


# --------------------------------------------------------------- at_coefficient ----
TARGETS = ("max_fast", "first_redo", "max_nowrap", "first_wrap", "first_scaled")
# encrypt calls redone for a ciphertext of each target (CKKS.encode_redo_count)
REDO = {"max_fast": 0, "first_redo": 1, "max_nowrap": 1, "first_wrap": 1, "first_scaled": 1}

Const = collections.namedtuple("Const", "c coeff log_approx")


@functools.lru_cache(maxsize=256)
def _coeff0(c, N, S, delta):
    co, la = O.encode_coeffs_ex(np.full(S, c), N, S, delta)
    assert np.count_nonzero(co[1:]) == 0, "a constant vector is the constant polynomial"
    return int(co[0]), la


def _largest(c0, ok):
    """The largest double c > 0 with ok(c), ok being true below some point and false above; c0 is
    within a few ulps of that point."""
    c, steps = c0, 0
    if ok(c):
        while ok(np.nextafter(c, np.inf)):
            c, steps = np.nextafter(c, np.inf), steps + 1
            assert steps < 64
    else:
        while not ok(c):
            c, steps = np.nextafter(c, -np.inf), steps + 1
            assert steps < 64
    return float(c)


@functools.lru_cache(maxsize=None)
def at_coefficient(N, S, delta, target):
    """The constant c > 0 that puts coefficient 0 at `target`, with the coefficient and the exponent
    the oracle gave for it (-c gives the negated coefficient):
      max_fast      the largest c with coefficient <= 2^61: the fast path's largest legal m
      first_redo    the next double up: redone with logApprox = 0
      max_nowrap    the largest c that FitToNativeVector leaves alone (2^62 - 512)
      first_wrap    the next double up: wrapped by -(2^63 - 513), still logApprox = 0
      first_scaled  the first c with logApprox = 1"""
    def f(c):
        return _coeff0(c, N, S, delta)

    up = lambda c: float(np.nextafter(c, np.inf))  # noqa: E731
    if target in ("max_fast", "first_redo"):
        c = _largest(2.0 ** 61 / delta, lambda c: f(c)[1] == 0 and 0 < f(c)[0] <= 2 ** 61)
        c = c if target == "max_fast" else up(c)
    elif target in ("max_nowrap", "first_wrap"):
        c = _largest(2.0 ** 62 / delta, lambda c: f(c)[1] == 0 and f(c)[0] > 0)
        c = c if target == "max_nowrap" else up(c)
    elif target == "first_scaled":
        c = up(_largest(2.0 ** 62 / delta * (1 + 2.0 ** -50), lambda c: f(c)[1] == 0))
    else:
        raise ValueError(target)
    co, la = f(c)
    return Const(c, co, la)


def constant(S, c):
    return np.full(S, float(c))


# ------------------------------------------------------------- huge / overflow ----
HUGE = 1e290      # logApprox about 950: ldexp(1.0, la), 2^la mod q_t and the division by 2^la
OVERFLOW = 1e300  # finite, but FFTSpecialInv(x)_i / S * Delta is not


def huge(S, every_slot):
    """1e290 in one slot (the rest uniform(-1, 1), which then rounds to 0) or in every slot."""
    if every_slot:
        return np.full(S, HUGE)
    x = np.random.default_rng(77).uniform(-1, 1, S)
    x[S // 5] = HUGE
    return x


def overflow(S, delta):
    """1e300 in one slot: a / S * Delta is infinite at a 52-bit scale; the shorter scaling primes need
    1.5e308 for that (Delta / S is 2^18 .. 2^29 there)."""
    a = OVERFLOW if np.isinf(OVERFLOW / S * (delta * 0.25)) else 1.5e308
    assert np.isinf(a / S * (delta * 0.25))  # with room for a position's |cos| or |sin|
    x = np.random.default_rng(78).uniform(-1, 1, S)
    x[S // 7] = a
    return x
