"""tests/encode_edge_inputs.py's builders land where they claim, on every context shape that
tests/test_gpu_encode_edge.py runs them on: judged by the oracle's encode (or_encode_coeffs_ex) and by an
exact restatement of the rounding and of FitToNativeVector's wrap in Python integers.  Without this the
GPU tests could pass for the wrong reason (a "2^61" input that never reaches 2^60, as
tests/test_gpu_encode_large.py's first cases turned out to be).

Also the decode on the CPU: O.decrypt_vector(O.encrypt_vector(x)) is within 2^-40 max|x| of x for every
input whose coefficients are neither wrapped nor scaled past the modulus (the bound
tests/test_gpu_encode_large.py derives from the 62 bits the scale-down keeps), so the GPU tests need
equality with the oracle only.  The wrapped constants and 1e290 (coefficient 2^logApprox far above Q) do
not decrypt to x, here or in PALISADE; for them the oracle's encrypt and decrypt must merely run."""
from fractions import Fraction

import numpy as np
import pytest

import encode_edge_inputs as E
import oracle as O

B = 2 ** 63 - 513  # PALISADE's Max64BitValue()
NAMES = list(E.SHAPES)


def _fit_wrap_ref(r):
    temp = B + r if r < 0 else r
    return temp - B if temp > B >> 1 else temp


def _llround(y):
    return int(abs(y) + Fraction(1, 2)) * (1 if y >= 0 else -1)  # ties away from zero


_KEYS = {}


def _keys(name):
    if name not in _KEYS:
        ch = E.chain(name)
        rng = np.random.default_rng(len(name))
        s = rng.integers(-1, 2, ch.N).astype(np.int64)
        e = rng.integers(-3, 4, ch.N).astype(np.int64)
        a = np.stack([rng.integers(0, int(qt), ch.N, dtype=np.uint64) for qt in ch.q])
        _KEYS[name] = O.keygen(s, e, a, ch.q, ch.psi)
    return _KEYS[name]


def _round_trip(name, x):
    ch = E.chain(name)
    sk, pk = _keys(name)
    ct = O.encrypt_vector(x, pk, ch.q, ch.psi, ch.N, ch.S, ch.delta, seed=5)
    return O.decrypt_vector(ct, sk, ch.q, ch.psi, ch.S, ch.delta, len(x))


def test_shapes_are_the_chains_the_gpu_tests_name():
    for name, bits in (("30-bit", [40, 31]), ("41-bit/2^13", [45, 42]), ("41-bit/2^15", [45, 42, 41, 42]),
                       ("2^15/L4", [60, 53, 52, 53])):
        assert [int(q).bit_length() for q in E.chain(name).q] == bits, name
    for name in NAMES:
        ch = E.chain(name)
        assert ch.N >= 2 * ch.S and ch.delta == float(int(ch.q[-1]))


@pytest.mark.parametrize("name", NAMES)
def test_dense_band(name):
    ch = E.chain(name)
    K = 3  # impulses at slots S - 1, 0 and 1, signs + - +
    x = E.dense_band(ch.S, ch.delta, K)
    assert E.impulse_slots(ch.S, K) == [ch.S - 1, 0, 1]
    assert len(set(E.impulse_slots(ch.S, 192))) == 192 and max(E.impulse_slots(ch.S, 192)[3:]) < ch.S - 3
    assert [x[k * ch.S + s] > 0 for k, s in enumerate(E.impulse_slots(ch.S, K))] == [True, False, True]
    gap = ch.N // (2 * ch.S)
    for k in range(K):
        c, la = O.encode_coeffs_ex(x[k * ch.S:(k + 1) * ch.S], ch.N, ch.S, ch.delta)
        assert la == 0
        a = np.abs(c.astype(np.float64))
        assert a.max() <= 2.0 ** 61 and a.max() > 0.98 * 2.0 ** 61
        band = np.concatenate([a[0:ch.N // 2:gap], a[ch.N // 2::gap]])
        assert band.size == 2 * ch.S and np.count_nonzero(a) == np.count_nonzero(band)
        assert np.count_nonzero(band > 2.0 ** 60) >= band.size // 2
    assert np.abs(_round_trip(name, x) - x).max() <= 2.0 ** -40 * np.abs(x).max()


@pytest.mark.parametrize("target", E.TARGETS)
@pytest.mark.parametrize("name", NAMES)
def test_at_coefficient(name, target):
    ch = E.chain(name)
    t = E.at_coefficient(ch.N, ch.S, ch.delta, target)
    below = E._coeff0(float(np.nextafter(t.c, 0)), ch.N, ch.S, ch.delta)
    above = E._coeff0(float(np.nextafter(t.c, np.inf)), ch.N, ch.S, ch.delta)
    # where the target sits
    if target == "max_fast":
        assert t.log_approx == 0 and 2 ** 61 - 256 <= t.coeff <= 2 ** 61 < above[0]
    elif target == "first_redo":
        assert t.log_approx == 0 and below[0] <= 2 ** 61 < t.coeff <= 2 ** 61 + 1024
    elif target == "max_nowrap":
        assert t.log_approx == 0 and t.coeff == 2 ** 62 - 512 and above[0] < 0
    elif target == "first_wrap":
        assert t.log_approx == 0 and below[0] == 2 ** 62 - 512
        assert t.coeff in (2 ** 62 - B, 2 ** 62 + 1024 - B)  # -(2^62 - 513), -(2^62 - 1537)
    else:
        assert t.log_approx == 1 and below[1] == 0 and 2 ** 61 < t.coeff < 2 ** 61 + 2 ** 14
    if name in ("2^13/L2", "2^15/L4"):  # the default scaling prime 0x10000000060001
        want = {"max_fast": 2 ** 61, "first_redo": 2 ** 61 + 512, "max_nowrap": 2 ** 62 - 512,
                "first_wrap": -(2 ** 62 - 513)}
        assert target == "first_scaled" or t.coeff == want[target]
    # the oracle's coefficient is the exact rounding of fl(c * Delta) / 2^logApprox, wrapped; both signs
    for sign in (1, -1):
        got = E._coeff0(sign * t.c, ch.N, ch.S, ch.delta)
        v = Fraction(sign * t.c * ch.delta)  # the binary64 product, as the encode forms it
        assert got == (_fit_wrap_ref(_llround(v / 2 ** t.log_approx)), t.log_approx)
        assert got[0] == sign * t.coeff
        x = E.constant(ch.S, sign * t.c)
        dec = _round_trip(name, x)
        if target != "first_wrap":
            assert np.abs(dec - x).max() <= 2.0 ** -40 * t.c


@pytest.mark.parametrize("name", NAMES)
def test_huge_and_overflow(name):
    ch = E.chain(name)
    for every in (False, True):
        x = E.huge(ch.S, every)
        c, la = O.encode_coeffs_ex(x, ch.N, ch.S, ch.delta)
        assert la > 900 and 2 ** 61 <= int(np.abs(c).max()) <= 2 ** 62
        assert np.all(np.isfinite(_round_trip(name, x)))  # the GPU tests' reference exists
    x = E.overflow(ch.S, ch.delta)
    assert x.max() == (1e300 if E.SHAPES[name][3] == 52 else 1.5e308)
    assert np.all(np.isfinite(x))
    with pytest.raises(ValueError):
        O.encode_coeffs_ex(x, ch.N, ch.S, ch.delta)
    sk, pk = _keys(name)
    with pytest.raises(ValueError):
        O.encrypt_vector(x, pk, ch.q, ch.psi, ch.N, ch.S, ch.delta, seed=5)
