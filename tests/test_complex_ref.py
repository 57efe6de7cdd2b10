"""Complex slot packing and conjugation without a device: the yardstick the GPU tests
measure the kernels with (tests/complex_ref.py) checked for what it must mean.

encode_complex with zero imaginary parts is O.encode bit for bit, on the normal and on the scale-down path;
decode_complex's real parts are O.decrypt bit for bit; an encode -> O.encrypt -> decode round trip returns both
halves of every slot; conj_ref decrypts to the complex conjugate at full and sparse packing; and the gather
form of g = 2N - 1 is the coefficient-domain definition on every ring."""
import functools

import numpy as np
import pytest

import complex_ref as X
import oracle as O
import rotation_ref as R

N, L, SEED = 1 << 11, 2, 91


@functools.lru_cache(maxsize=None)
def _keys():
    q, psi = O.params_generate(N, L, 52, 60)
    s, e, a = O.sample_keygen(SEED, N, q)
    sk, pk = O.keygen(s, e, a, q, psi)
    evk = O.evk_keygen(SEED, sk, q, psi)
    return q, psi, sk, pk, evk


@pytest.mark.parametrize("slots", [N // 2, N // 8, 8], ids=["full", "sparse", "tiny"])
def test_zero_imaginary_parts_encode_as_the_oracle_does(slots):
    q, psi = _keys()[:2]
    delta = float(q[-1])
    rng = np.random.default_rng(slots)
    for n in (slots, slots - 1, 1):
        x = rng.uniform(-4, 4, n)
        z = np.zeros(2 * n)
        z[0::2] = x  # interleaved, every imaginary part 0
        assert np.array_equal(X.encode_complex(z, N, slots, delta, q, psi), O.encode(x, N, slots, delta, q, psi))
        c, a = X.encode_coeffs_complex(X.pairs(z, slots), N, slots, delta)
        assert a == 0 and np.array_equal(c, O.encode_coeffs(x, N, slots, delta))


def test_scale_down_path_matches_the_oracle_and_takes_its_maximum_over_both_parts():
    q, psi = _keys()[:2]
    delta, slots = float(q[-1]), N // 4
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, slots)
    x[3] = 2.0 ** 30  # |x Delta| about 2^82: logApprox about 20
    z = np.zeros(2 * slots)
    z[0::2] = x
    c, a = X.encode_coeffs_complex(X.pairs(z, slots), N, slots, delta)
    co, ao = O.encode_coeffs_ex(x, N, slots, delta)
    assert a == ao > 0 and np.array_equal(c, co)
    assert np.array_equal(X.encode_complex(z, N, slots, delta, q, psi), O.encode(x, N, slots, delta, q, psi))
    # the same magnitude in an imaginary part alone forces the same exponent (or_encode_coeffs_ex's rule over
    # re and im): i x encodes as the coefficients of x moved to the other half, so the exponents agree
    zi = np.zeros(2 * slots)
    zi[1::2] = x
    ci, ai = X.encode_coeffs_complex(X.pairs(zi, slots), N, slots, delta)
    assert ai == ao
    small = np.zeros(2 * slots)
    small[1::2] = rng.uniform(-1, 1, slots)
    assert X.encode_coeffs_complex(X.pairs(small, slots), N, slots, delta)[1] == 0
    # rounding helpers against the oracle's scalar forms, at their edges
    for v in (0.5, -0.5, 1.5, -2.5, 0.49999999999999994, 2.0 ** 61 + 1024, -(2.0 ** 62)):
        assert X.round_half_away(np.array([v]))[0] == O.lib.or_round_half_away(v)
    for r in (0, 1, -1, X.MAX64 >> 1, (X.MAX64 >> 1) + 1, -(X.MAX64 >> 1) - 256, -(X.MAX64 >> 1) - 257, 1 << 62,
              -(1 << 62)):
        assert X.fit_wrap(np.array([r], np.int64))[0] == O.lib.or_fit_wrap(r), r


@pytest.mark.parametrize("slots", [N // 2, N // 8], ids=["full", "sparse"])
def test_round_trip_returns_both_halves_and_the_real_parts_are_the_oracles(slots):
    q, psi, sk, pk, _ = _keys()
    delta = float(q[-1])
    rng = np.random.default_rng(7 + slots)
    V = 2 * slots
    x = rng.uniform(-1, 1, V + 3)  # K = 2, the second ciphertext nearly empty
    ct = X.encrypt_vector_complex(x, pk, q, psi, N, slots, delta, SEED)
    assert ct.shape == (2, 2, L, N)
    dec = X.decode_vector_complex(ct, sk, q, psi, slots, delta, len(x))
    # the real round trip on the same context, the same seed and the even-indexed values: its error x 4 is the
    # bound for both parts (each carries the same rounding and the same encryption noise)
    ctr = O.encrypt_vector(x[:V][0::2], pk, q, psi, N, slots, delta, SEED)
    real_err = np.abs(O.decrypt_vector(ctr, sk, q, psi, slots, delta, slots) - x[:V][0::2]).max()
    err = np.abs(dec - x).max()
    print("complex round trip slots=%d: max error %.3g, real round trip %.3g" % (slots, err, real_err))
    assert 0 < real_err and err <= 4 * real_err
    # decode_complex's real parts equal O.decrypt bit for bit, whatever the ciphertext holds
    for k in range(2):
        full = X.decode_complex(ct[k], sk, q, psi, slots, delta)
        assert np.array_equal(full[0::2], O.decrypt(ct[k], sk, q, psi, slots, delta, slots))
    # values beyond n were encoded as 0
    tail = X.decode_complex(ct[1], sk, q, psi, slots, delta)[3:]
    assert np.abs(tail).max() <= 4 * real_err


@pytest.mark.parametrize("slots", [N // 2, N // 8], ids=["full", "sparse"])
def test_reference_conjugation_decrypts_to_the_conjugate(slots):
    q, psi, sk, pk, evk = _keys()
    delta = float(q[-1])
    rng = np.random.default_rng(11 + slots)
    x = rng.uniform(-1, 1, 4 * slots)  # K = 2
    ct = X.encrypt_vector_complex(x, pk, q, psi, N, slots, delta, SEED)
    key = X.conj_key_from_evk(evk, sk, q, psi)
    e = X.key_error_g(key, X.conj_galois(N), sk, q, psi)
    assert np.abs(e).max() < 64 and e.any() and (e == e[:, :1]).all()
    out = X.conj_ref(ct, key, q, psi)
    dec = X.decode_vector_complex(out, sk, q, psi, slots, delta, len(x))
    exp = x.copy()
    exp[1::2] = -exp[1::2]
    assert np.abs(dec - exp).max() < 1e-7
    # a real-packed ciphertext is fixed by conjugation, up to the key switch's noise
    xr = rng.uniform(-1, 1, slots)
    cr = O.encrypt_vector(xr, pk, q, psi, N, slots, delta, SEED)
    assert np.abs(O.decrypt_vector(X.conj_ref(cr, key, q, psi), sk, q, psi, slots, delta, slots) - xr).max() < 1e-7


@pytest.mark.parametrize("logn", range(11, 18))
def test_gather_form_of_conjugation(logn):
    """R.gather_index(N, 2N - 1) against the coefficient-domain definition (one tower, one random polynomial)."""
    n = 1 << logn
    q, psi = O.params_generate(n, 1, 52, 60)
    g = X.conj_galois(n)
    x = np.random.default_rng(logn).integers(0, int(q[0]), n, dtype=np.uint64)
    src = R.gather_index(n, g)
    assert np.array_equal(np.sort(src), np.arange(n))
    assert np.array_equal(x[src], R.sigma_eval(x[None], g, q, psi)[0])
    assert np.array_equal(src[src], np.arange(n))  # an involution
