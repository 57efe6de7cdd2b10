"""Reference for complex slot packing and conjugation, built from the oracle's parts only.

encode_complex: O.fft_special_inv on the complex slot vector, then the rounding and placement of
oracle/ckks_oracle.c's or_encode_coeffs_ex restated in numpy (the scale-down exponent over both parts, llround
with ties away from zero, FitToNativeVector's wrap, real part at i gap and imaginary part at N/2 + i gap), the
per-tower residues times 2^logApprox, and O.ntt_fwd.  With zero imaginary parts it is O.encode
(tests/test_complex_ref.py).  decode_complex: O.decrypt_coeffs, then O.fft_special, both parts kept.
conj_ref: tests/rotation_ref.py's rotate_ref at the Galois element 2N - 1.

Test infrastructure only; nothing here is imported by the product."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle as O
import rotation_ref as R

MAX_BITS_IN_WORD = 62
MAX64 = (1 << 63) - 513  # PALISADE's Max64BitValue()


def pairs(x, slots):
    """n interleaved values -> the slot vector of one ciphertext: z[s] = x[2 s] + i x[2 s + 1], values at or
    beyond n read as 0."""
    x = np.asarray(x, np.float64)
    assert len(x) <= 2 * slots
    v = np.zeros(2 * slots, np.float64)
    v[:len(x)] = x
    return v[0::2] + 1j * v[1::2]


def round_half_away(v):
    """or_round_half_away on an array."""
    t = np.trunc(v)
    d = v - t
    t = np.where(d >= 0.5, t + 1.0, np.where(d <= -0.5, t - 1.0, t))
    return t.astype(np.int64)


def fit_wrap(r):
    """or_fit_wrap on an int64 array."""
    r = np.asarray(r, np.int64)
    hf = MAX64 >> 1
    out = r.copy()
    hi = r > hf
    out[hi] = r[hi] - MAX64
    lo = (r < 0) & (r <= hf - MAX64)  # MAX64 + r <= hf, without the overflow
    out[lo] = r[lo] + MAX64
    return out


def encode_coeffs_complex(z, N, slots, delta):
    """or_encode_coeffs_ex on a complex slot vector z [slots] -> (signed coefficients [N], logApprox)."""
    z = np.asarray(z, np.complex128)
    assert len(z) == slots and 2 * slots <= N
    f = O.fft_special_inv(z)
    re, im = f.real * float(delta), f.imag * float(delta)
    if not (np.isfinite(re).all() and np.isfinite(im).all()):
        raise ValueError("encode: non-finite value")
    # the maximum of ceil(log2 |v|) over the nonzero values of both parts, at least 0: taken at the largest
    # |v| with the oracle's own log2 (ceil(log2) is monotone in |v|)
    big = max(np.abs(re).max(), np.abs(im).max())
    logc = max(0, int(O.lib.or_encode_logc(float(big)))) if big != 0 else 0
    a = logc - MAX_BITS_IN_WORD if logc > MAX_BITS_IN_WORD else 0
    approx = np.ldexp(1.0, a)
    gap = N // (2 * slots)
    c = np.zeros(N, np.int64)
    c[0:slots * gap:gap] = fit_wrap(round_half_away(re / approx))
    c[N // 2:N // 2 + slots * gap:gap] = fit_wrap(round_half_away(im / approx))
    return c, a


def residues(c, a, q, psi):
    """or_encode's second half: coefficients times 2^a mod q_t, then the forward NTT -> [L][N]."""
    out = np.zeros((len(q), len(c)), np.uint64)
    for t in range(len(q)):
        qt = int(q[t])
        r = np.mod(c, np.int64(qt)).astype(np.uint64)  # or_mod_signed
        if a:
            r = R.mulmod(r, np.uint64(pow(2, a, qt)), qt)
        out[t] = O.ntt_fwd(r, qt, int(psi[t]))
    return out


def encode_complex(x, N, slots, delta, q, psi):
    """The plaintext [L][N] (EVALUATION) of one ciphertext's n <= 2 slots interleaved values."""
    c, a = encode_coeffs_complex(pairs(x, slots), N, slots, delta)
    return residues(c, a, q, psi)


def encode_vector_complex(x, N, slots, delta, q, psi):
    """n values -> K = ceil(n / V) plaintexts [K][L][N], V = 2 slots."""
    x = np.asarray(x, np.float64)
    V = 2 * slots
    K = -(-len(x) // V)
    return np.stack([encode_complex(x[k * V:(k + 1) * V], N, slots, delta, q, psi) for k in range(K)])


def encrypt_vector_complex(x, pk, q, psi, N, slots, delta, seed, g0=0):
    """O.encrypt_vector with the restated plaintext: ciphertext k under O.sample_encrypt's stream g0 + k."""
    pts = encode_vector_complex(x, N, slots, delta, q, psi)
    out = np.zeros((len(pts), 2, len(q), N), np.uint64)
    for k, m in enumerate(pts):
        v, e0, e1 = O.sample_encrypt(seed, g0 + k, N)
        out[k] = O.encrypt(pk, m, v, e0, e1, q, psi)
    return out


def decode_complex(ct, sk, q, psi, slots, scale):
    """One ciphertext [2][l][N] -> its 2 slots interleaved values: FFTSpecial(re + i im), both parts."""
    re, im = O.decrypt_coeffs(ct, sk, q, psi, slots, scale)
    z = O.fft_special(re + 1j * im)
    out = np.empty(2 * slots, np.float64)
    out[0::2], out[1::2] = z.real, z.imag
    return out


def decode_vector_complex(cts, sk, q, psi, slots, scale, n):
    """The first n values of K ciphertexts (ciphertexts past ceil(n / V) are not read)."""
    V = 2 * slots
    K = -(-n // V)
    if not K:
        return np.zeros(0)
    l = cts.shape[2]
    out = np.concatenate([decode_complex(cts[k], sk[:l], q[:l], psi[:l], slots, scale) for k in range(K)])
    return out[:n]


def conj_galois(N):
    return 2 * N - 1


def galois_apply_ref(ct, g, key, q, psi):
    """tests/rotation_ref.py's rotate_ref at a Galois element given directly: (sigma_g(c0) + u0, u1), (u0, u1) =
    KeySwitch(sigma_g(c1)) under `key`; ct [K][2][l][N]."""
    ct = np.asarray(ct, np.uint64)
    K, _, l, N = ct.shape
    ql = np.asarray(q[:l], np.uint64)[:, None]

    def one(k):
        s = R.sigma_eval(ct[k], g, q, psi)
        X, Y = np.zeros((1, 2, l, N), np.uint64), np.zeros((1, 2, l, N), np.uint64)
        X[0, 1] = s[1]
        Y[0, 1] = 1  # the constant 1 in EVALUATION: R.rotate_ref's O.eval_mult trick
        out = O.eval_mult(X, Y, key, q, psi)[0]
        out[0] = (out[0] + s[0]) % ql
        return out

    with ThreadPoolExecutor(max_workers=max(1, min(K, 8))) as pool:
        return np.stack(list(pool.map(one, range(K))))


def conj_ref(ct, key, q, psi):
    return galois_apply_ref(ct, conj_galois(np.asarray(ct).shape[-1]), key, q, psi)


def key_error_g(key, g, sk, q, psi):
    """R.key_error at a Galois element given directly."""
    key = np.asarray(key, np.uint64)
    _, dn, T, N = key.shape
    L = len(q)
    _, al, _, _ = O.special_primes(N, q)
    S, mods, roots = R.s_ext(sk, q, psi)
    sig = R.sigma_eval(S[:L], g, q, psi)
    pm = R.p_mod(q, N)
    out = np.zeros((dn, T, N), np.int64)
    for j in range(dn):
        for t in range(T):
            m = np.uint64(mods[t])
            v = (key[0, j, t] + R.mulmod(key[1, j, t], S[t], m)) % m
            if t < L and j * al <= t < (j + 1) * al:
                v = (v + m - R.mulmod(np.uint64(pm[t]), sig[t], m)) % m
            out[j, t] = O.to_signed(O.ntt_inv(v, mods[t], roots[t]), mods[t])
    return out


def conj_key_from_evk(evk, sk, q, psi):
    """R.rot_key_from_evk at g = 2N - 1: a conjugation key for tests that have no device."""
    key = np.array(evk, np.uint64)
    _, dn, T, N = key.shape
    L = len(q)
    _, al, _, _ = O.special_primes(N, q)
    sk = np.asarray(sk, np.uint64)
    sig = R.sigma_eval(sk, conj_galois(N), q, psi)
    pm = R.p_mod(q, N)
    for j in range(dn):
        for t in range(j * al, min(L, (j + 1) * al)):
            m = np.uint64(q[t])
            s2 = R.mulmod(np.uint64(pm[t]), R.mulmod(sk[t], sk[t], m), m)
            key[0, j, t] = (key[0, j, t] + m - s2 + R.mulmod(np.uint64(pm[t]), sig[t], m)) % m
    return key
