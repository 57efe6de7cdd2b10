"""Reference for slot rotations and EvalSum, built from the oracle's parts only:
the automorphism in the coefficient domain between O.ntt_inv and O.ntt_fwd, and the HYBRID key
switch as O.eval_mult of (0, sigma(c1)) by (0, 1) -- its tensor terms c0, c1 vanish and c2 is
sigma(c1), so it returns exactly KeySwitch(sigma(c1)) under any key in the evaluation key's layout.

Test infrastructure only; nothing here is imported by the product."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle as O


def galois(N, r):
    """g = 5^r mod 2N, the inverse for r < 0 (PALISADE's FindAutomorphismIndex2nComplex)."""
    g = pow(5, abs(int(r)), 2 * N)
    return pow(g, -1, 2 * N) if r < 0 else g


def mulmod(a, b, q):
    """a b mod q for uint64 arrays below q < 2^60: 4 bits of a at a time, every intermediate < 2^64."""
    a, b, q = np.asarray(a, np.uint64), np.asarray(b, np.uint64), np.uint64(q)
    r = np.zeros(np.broadcast(a, b).shape, np.uint64)
    for sh in range(56, -4, -4):
        limb = (a >> np.uint64(sh)) & np.uint64(15)
        r = ((r << np.uint64(4)) % q + (limb * b) % q) % q
    return r


def sigma_coeff(a, g, q):
    """sigma_g on coefficients: coefficient i moves to i g mod 2N, negated when that is >= N."""
    a = np.asarray(a, np.uint64)
    N = len(a)
    d = (np.arange(N, dtype=np.int64) * int(g)) % (2 * N)
    out = np.zeros(N, np.uint64)
    out[d % N] = np.where(d >= N, (np.uint64(q) - a) % np.uint64(q), a)
    return out


def sigma_eval(x, g, q, psi):
    """sigma_g on polynomials in EVALUATION: x [..., l, N] over towers q[:l]."""
    x = np.asarray(x, np.uint64)
    out = np.empty_like(x)
    l = x.shape[-2]
    for idx in np.ndindex(*x.shape[:-1]):
        t = idx[-1]
        assert t < l
        out[idx] = O.ntt_fwd(sigma_coeff(O.ntt_inv(x[idx], q[t], psi[t]), g, q[t]), q[t], psi[t])
    return out


def gather_index(N, g):
    """The same automorphism as a gather in the NTT's own order: out[j] = in[src[j]],
    2 brev(src[j]) + 1 = g (2 brev(j) + 1) mod 2N."""
    logN = N.bit_length() - 1
    j = np.arange(N, dtype=np.int64)

    def brev(v):
        r = np.zeros_like(v)
        for i in range(logN):
            r |= ((v >> i) & 1) << (logN - 1 - i)
        return r

    return brev(((int(g) * (2 * brev(j) + 1)) % (2 * N)) >> 1)


def sweep_indices(batch):
    """The rotation indices the permutation sweeps run at a batch size (tests/test_gpu_rotate_gather.py,
    tests/test_rotation_ref.py): the small ones of both signs, those around batch / 2 and batch / 4,
    the largest, and sixteen more drawn from a seeded generator over (-batch, batch), none 0 or repeated."""
    fixed = [1, -1, 2, -2, 3, -3, 7, -7, batch // 2, batch // 2 + 1, batch // 2 - 1, batch // 4 + 1,
             batch - 1, -(batch - 1), batch - 2]
    rng = np.random.default_rng([20, batch])
    more = []
    while len(more) < 16:
        r = int(rng.integers(1 - batch, batch))
        if r and r not in fixed and r not in more:
            more.append(r)
    return fixed + more


def rotate_ref(ct, r, key, q, psi):
    """Rotate(ct, r) at ct's level: (sigma(c0) + u0, u1), (u0, u1) = KeySwitch(sigma(c1)) under `key`
    ([2][dnum][L + kP][N]); ct [K][2][l][N], q / psi the whole chain."""
    ct = np.asarray(ct, np.uint64)
    K, _, l, N = ct.shape
    g = galois(N, r)
    ql = np.asarray(q[:l], np.uint64)[:, None]

    def one(k):
        s = sigma_eval(ct[k], g, q, psi)
        X, Y = np.zeros((1, 2, l, N), np.uint64), np.zeros((1, 2, l, N), np.uint64)
        X[0, 1] = s[1]
        Y[0, 1] = 1  # the constant 1 in EVALUATION
        out = O.eval_mult(X, Y, key, q, psi)[0]
        out[0] = (out[0] + s[0]) % ql
        return out

    # the ciphertexts are independent and the oracle's C calls release the interpreter lock
    with ThreadPoolExecutor(max_workers=max(1, min(K, 8))) as pool:
        return np.stack(list(pool.map(one, range(K))))


def eval_sum_ref(ct, n, keys, q, psi):
    """EvalSum(ct, n): acc <- acc + Rotate(acc, 2^i), i < log2(n); keys: {index: key}."""
    acc = np.array(ct, np.uint64)
    ql = np.asarray(q[:acc.shape[2]], np.uint64)[:, None]
    r = 1
    while r < n:
        acc = (acc + rotate_ref(acc, r, keys[r], q, psi)) % ql
        r *= 2
    return acc


def s_ext(sk, q, psi):
    """s over Q u P in EVALUATION, [L + kP][N], from tower 0 of sk as or_evk_keygen derives it;
    -> (s_ext, moduli, roots) of the extended basis."""
    sk = np.asarray(sk, np.uint64)
    N = sk.shape[1]
    _, _, p, pr = O.special_primes(N, q)
    mods = [int(v) for v in q] + [int(v) for v in p]
    roots = [int(v) for v in psi] + [int(v) for v in pr]
    s = O.to_signed(O.ntt_inv(sk[0], q[0], psi[0]), int(q[0]))
    out = np.zeros((len(mods), N), np.uint64)
    for t, (m, w) in enumerate(zip(mods, roots)):
        out[t] = O.ntt_fwd((s % m).astype(np.uint64), m, w)
    return out, mods, roots


def p_mod(q, N):
    """P mod q_t for every tower of Q."""
    _, _, p, _ = O.special_primes(N, q)
    out = []
    for qt in q:
        v = 1
        for pm in p:
            v = v * int(pm) % int(qt)
        out.append(v)
    return out


def key_error(key, r, sk, q, psi):
    """The error polynomials a rotation key of index r hides: for every digit j and tower t of Q u P,
    INTT(b + a s_t - [t in digit j] P sigma_g(s)_t), centred; -> int64 [dnum][L + kP][N]."""
    key = np.asarray(key, np.uint64)
    _, dn, T, N = key.shape
    L = len(q)
    _, al, _, _ = O.special_primes(N, q)
    g = galois(N, r)
    S, mods, roots = s_ext(sk, q, psi)
    sig = sigma_eval(S[:L], g, q, psi)
    pm = p_mod(q, N)
    out = np.zeros((dn, T, N), np.int64)
    for j in range(dn):
        for t in range(T):
            m = np.uint64(mods[t])
            v = (key[0, j, t] + mulmod(key[1, j, t], S[t], m)) % m
            if t < L and j * al <= t < (j + 1) * al:
                v = (v + m - mulmod(np.uint64(pm[t]), sig[t], m)) % m
            out[j, t] = O.to_signed(O.ntt_inv(v, mods[t], roots[t]), mods[t])
    return out


def rot_key_from_evk(evk, r, sk, q, psi):
    """A rotation key for tests that have no device: the oracle's evaluation key with P s^2 replaced
    by P sigma_g(s) in every digit's own towers (its (a, e) pairs are the EvalMult key's, which a real
    key must never share: the product draws them from a stream domain of their own)."""
    key = np.array(evk, np.uint64)
    _, dn, T, N = key.shape
    L = len(q)
    _, al, _, _ = O.special_primes(N, q)
    g = galois(N, r)
    sk = np.asarray(sk, np.uint64)
    sig = sigma_eval(sk, g, q, psi)
    pm = p_mod(q, N)
    for j in range(dn):
        for t in range(j * al, min(L, (j + 1) * al)):
            m = np.uint64(q[t])
            s2 = mulmod(np.uint64(pm[t]), mulmod(sk[t], sk[t], m), m)
            key[0, j, t] = (key[0, j, t] + m - s2 + mulmod(np.uint64(pm[t]), sig[t], m)) % m
    return key
