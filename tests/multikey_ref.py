"""Reference for the multiparty evaluation-key protocols of threshold CKKS (the
reference's code/mkhe/mkhe.cpp:271-317), restated in numpy over the oracle's parts only: O.ntt_fwd /
O.ntt_inv, R.s_ext, R.sigma_eval, R.p_mod, R.mulmod for the arithmetic, and the ChaCha20 stream
(O.chacha20_block through the oracle's own word reader, O.seed_to_key, O.gauss_cdt) for the error
polynomials and the lead party's uniform a.

Keys are [2][dnum][L + kP][N] uint64 (b-vector, a-vector), EVALUATION.  tests/test_multikey_ref.py holds
this file to its meaning.  Test infrastructure only; nothing here is imported by the product."""
import ctypes as C

import numpy as np

import oracle as O
import rotation_ref as R

B_ERR = 64  # |e| < 64: the CDT has 43 entries (the key-structure tests' bound)


def stream_words(key, nonce, cnt):
    """u64 words [0, cnt) of the stream (key, nonce): word k of ChaCha20 block c is its 32-bit words
    2k, 2k + 1 (low first), blocks counted from 0 -- the oracle's reader over or_chacha20_block."""
    key = np.ascontiguousarray(key, dtype=np.uint32)
    out = np.zeros(cnt, np.uint64)
    O.lib.or_stream_words(key.ctypes.data_as(O.u32p), C.c_uint64(int(nonce)), C.c_uint64(0), cnt,
                          out.ctypes.data_as(O.u64p))
    return out


def gauss_errors(key, nonce, N):
    """One error polynomial: word i -> sign w & 1, |e| = #{k : (w >> 1) >= cdt[k]} (gauss_sample)."""
    w = stream_words(key, nonce, N)
    k = np.searchsorted(O.gauss_cdt(), w >> np.uint64(1), side="right").astype(np.int64)
    return np.where((w & np.uint64(1)).astype(bool), -k, k)


def uniform_a(key, nonce, N, m):
    """A uniform polynomial mod m: word pair (2i, 2i + 1) = (lo, hi) -> (hi 2^64 + lo) mod m."""
    w = stream_words(key, nonce, 2 * N)
    lo, hi = w[0::2], w[1::2]
    mm = np.uint64(m)
    r64 = np.uint64((1 << 64) % int(m))
    return (R.mulmod(hi % mm, r64, mm) + lo % mm) % mm


def sample_digit(key, base, j, N, mods, with_a=True):
    """evk_sample_kernel's draw for digit j under a nonce base: e (int64 [N], nonce base | j << 16) and
    a ([T][N], nonce base | j << 16 | 1 + t)."""
    nonce = int(base) | (j << 16)
    e = gauss_errors(key, nonce, N)
    a = np.stack([uniform_a(key, nonce | (1 + t), N, m) for t, m in enumerate(mods)]) if with_a else None
    return e, a


def _ntt_small(e, mods, roots):
    return np.stack([O.ntt_fwd((e % m).astype(np.uint64), m, w) for m, w in zip(mods, roots)])


def _dims(sk, q):
    N = np.asarray(sk).shape[1]
    dn, al, p, _ = O.special_primes(N, q)
    return N, len(q), dn, al, len(q) + len(p)


def share(seed, sk, q, psi, index=0, prev=None):
    """Round 1: party's share of the key of `index` (0: the EvalMult share, s' = s; else the rotation
    share, s' = sigma_g(s)).  prev=None: the lead party draws a; else a is prev's a-vector."""
    N, L, dn, al, T = _dims(sk, q)
    key = O.seed_to_key(seed)
    S, mods, roots = R.s_ext(sk, q, psi)
    g = 1 if index == 0 else R.galois(N, index)
    sp = S[:L] if g == 1 else R.sigma_eval(S[:L], g, q, psi)
    pm = R.p_mod(q, N)
    out = np.zeros((2, dn, T, N), np.uint64)
    for j in range(dn):
        e, a = sample_digit(key, (7 << 56) | (g << 24), j, N, mods, with_a=prev is None)
        if prev is not None:
            a = np.asarray(prev, np.uint64)[1, j]
        E = _ntt_small(e, mods, roots)
        for t in range(T):
            m = np.uint64(mods[t])
            b = (E[t] + m - R.mulmod(a[t], S[t], m)) % m
            if t < L and j * al <= t < (j + 1) * al:
                b = (b + R.mulmod(np.uint64(pm[t]), sp[t], m)) % m
            out[0, j, t], out[1, j, t] = b, a[t]
    return out


def key_add(keys, q, N, sum_a=False):
    """MultiAddEvalKeys / MultiAddEvalSumKeys (sum_a False: a-vectors equal, kept) and
    MultiAddEvalMultKeys (sum_a: both summed); up to 16 keys, residues below 2^60: no uint64 wrap."""
    keys = [np.asarray(k, np.uint64) for k in keys]
    assert 1 <= len(keys) <= 16
    _, _, p, _ = O.special_primes(N, q)
    mods = np.array([int(v) for v in q] + [int(v) for v in p], np.uint64)[:, None]
    out = np.empty_like(keys[0])
    out[0] = sum(k[0] for k in keys) % mods
    if sum_a:
        out[1] = sum(k[1] for k in keys) % mods
    else:
        assert all(np.array_equal(k[1], keys[0][1]) for k in keys)
        out[1] = keys[0][1]
    return out


def round2_errors(seed, N, dn):
    """Round 2's error polynomials, int64 [2][dnum][N]: vector v (0: b, 1: a), digit j."""
    key = O.seed_to_key(seed)
    return np.stack([np.stack([gauss_errors(key, (8 << 56) | (v << 24) | (j << 16), N) for j in range(dn)])
                     for v in range(2)])


def round2(seed, joint, sk, q, psi):
    """MultiMultEvalKey(joint, sk): out[v][j] = joint[v][j] s + NTT(E_{v,j})."""
    N, L, dn, al, T = _dims(sk, q)
    joint = np.asarray(joint, np.uint64)
    S, mods, roots = R.s_ext(sk, q, psi)
    E = round2_errors(seed, N, dn)
    out = np.empty_like(joint)
    for v in range(2):
        for j in range(dn):
            En = _ntt_small(E[v, j], mods, roots)
            for t in range(T):
                m = np.uint64(mods[t])
                out[v, j, t] = (R.mulmod(joint[v, j, t], S[t], m) + En[t]) % m
    return out


def sk_sum(sks, q):
    """sum s_i in EVALUATION, [L][N]."""
    qs = np.asarray(q, np.uint64)[:, None]
    tot = np.zeros_like(np.asarray(sks[0], np.uint64))
    for s in sks:
        tot = (tot + np.asarray(s, np.uint64)) % qs
    return tot


def switch_key_error(key, index, sk, q, psi):
    """The error a key hides: INTT(b + a s - [t in digit j] P s'), centred, int64 [dnum][L + kP][N];
    s' = s (index 0), s^2 (index "mult": an EvalMult key) or sigma_g(s) (a rotation index), as
    R.key_error extracts a rotation key's."""
    if index not in (0, "mult"):
        return R.key_error(key, index, sk, q, psi)
    key = np.asarray(key, np.uint64)
    _, dn, T, N = key.shape
    L = len(q)
    _, al, _, _ = O.special_primes(N, q)
    S, mods, roots = R.s_ext(sk, q, psi)
    pm = R.p_mod(q, N)
    out = np.zeros((dn, T, N), np.int64)
    for j in range(dn):
        for t in range(T):
            m = np.uint64(mods[t])
            v = (key[0, j, t] + R.mulmod(key[1, j, t], S[t], m)) % m
            if t < L and j * al <= t < (j + 1) * al:
                sp = S[t] if index == 0 else R.mulmod(S[t], S[t], m)
                v = (v + m - R.mulmod(np.uint64(pm[t]), sp, m)) % m
            out[j, t] = O.to_signed(O.ntt_inv(v, mods[t], roots[t]), mods[t])
    return out


def mult_key_bound(N, parties):
    """Worst case of the final EvalMult key's |error| = |e s + E1 s + E2| per digit: e = sum of Pn
    round-1 errors (|.| < Pn B), s = sum of Pn ternary shares (|.| <= Pn), E1, E2 sums of Pn round-2
    errors: N (Pn B)(Pn) + N (Pn B)(Pn) + Pn B = B Pn (2 N Pn + 1)."""
    return B_ERR * parties * (2 * N * parties + 1)


def protocol(seeds, sks, q, psi, indices=()):
    """The whole protocol for parties seeded `seeds` holding `sks`: -> (final EvalMult key, {index:
    joint rotation key}, the round-1 EvalMult sum).  Party 0 leads; party i copies party i - 1's a."""
    N = np.asarray(sks[0]).shape[1]
    shares = []
    for sd, sk in zip(seeds, sks):
        shares.append(share(sd, sk, q, psi, 0, shares[-1] if shares else None))
    mid = key_add(shares, q, N)
    final = key_add([round2(sd, mid, sk, q, psi) for sd, sk in zip(seeds, sks)], q, N, sum_a=True)
    rot = {}
    for r in indices:
        rs = []
        for sd, sk in zip(seeds, sks):
            rs.append(share(sd, sk, q, psi, r, rs[-1] if rs else None))
        rot[r] = key_add(rs, q, N)
    return final, rot, mid


# ---- helpers of tests/test_gpu_multikey_edges.py (held to their meaning by tests/test_multikey_ref.py) ----
def ext_moduli(N, q):
    """The moduli of Q then of P, uint64 [L + kP]."""
    _, _, p, _ = O.special_primes(N, q)
    return np.array([int(v) for v in q] + [int(v) for v in p], np.uint64)


def uniform_key(rng, mods, dn, N):
    """A key [2][dnum][T][N] of residues uniform below each tower's modulus."""
    out = np.empty((2, dn, len(mods), N), np.uint64)
    for t, mt in enumerate(mods):
        out[:, :, t] = rng.integers(0, int(mt), size=(2, dn, N), dtype=np.uint64)
    return out


def full_key(mods, dn, N):
    """A key whose every word is q_t - 1."""
    out = np.empty((2, dn, len(mods), N), np.uint64)
    out[:] = (np.asarray(mods, np.uint64) - np.uint64(1))[None, None, :, None]
    return out


def chain_step(seed, prev_pk, q, psi):
    """MultipartyKeyGen(prev_pk) under `seed`: -> (pk, sk) with sk = NTT(s), pk = (prev.b + NTT(e) -
    prev.a sk, prev.a); s, e the oracle's keygen draw of that seed (its uniform a unused)."""
    prev = np.asarray(prev_pk, np.uint64)
    N = prev.shape[-1]
    s, e, _ = O.sample_keygen(seed, N, q)
    sk, pk = np.empty((len(q), N), np.uint64), np.empty((2, len(q), N), np.uint64)
    for t, (qt, pt) in enumerate(zip(q, psi)):
        m = np.uint64(qt)
        sk[t] = O.ntt_fwd((s % int(qt)).astype(np.uint64), qt, pt)
        ne = O.ntt_fwd((e % int(qt)).astype(np.uint64), qt, pt)
        pk[0, t] = (prev[0, t] + (ne + m - R.mulmod(prev[1, t], sk[t], m)) % m) % m
        pk[1, t] = prev[1, t]
    return pk, sk


def share_terms(seed, sk, q, psi, index=0):
    """What a follower's share holds besides prev: (C [dnum][T][N], S [T][N], mods) with C = NTT(e_j) +
    [t in digit j] (P mod q_t) s'; share(..., prev) = (C - prev.a S, prev.a).  For sweeps over many prev
    keys of one (seed, index): the NTTs are done once."""
    N, L, dn, al, T = _dims(sk, q)
    key = O.seed_to_key(seed)
    S, mods, roots = R.s_ext(sk, q, psi)
    g = 1 if index == 0 else R.galois(N, index)
    sp = S[:L] if g == 1 else R.sigma_eval(S[:L], g, q, psi)
    pm = R.p_mod(q, N)
    Cc = np.empty((dn, T, N), np.uint64)
    for j in range(dn):
        e, _ = sample_digit(key, (7 << 56) | (g << 24), j, N, mods, with_a=False)
        Cc[j] = _ntt_small(e, mods, roots)
        for t in range(j * al, min(L, (j + 1) * al)):
            m = np.uint64(mods[t])
            Cc[j, t] = (Cc[j, t] + R.mulmod(np.uint64(pm[t]), sp[t], m)) % m
    return Cc, S, mods


def share_from_terms(terms, prev):
    """share(seed, sk, q, psi, index, prev) from share_terms(seed, sk, q, psi, index)."""
    Cc, S, mods = terms
    a = np.asarray(prev, np.uint64)[1]
    out = np.empty((2,) + a.shape, np.uint64)
    for t, mt in enumerate(mods):
        m = np.uint64(mt)
        out[0, :, t] = (Cc[:, t] + m - R.mulmod(a[:, t], S[t], m)) % m
    out[1] = a
    return out


def round2_terms(seed, sk, q, psi):
    """(NTT(E) [2][dnum][T][N], S [T][N], mods): round2(seed, joint, ...) = joint S + NTT(E)."""
    N, L, dn, al, T = _dims(sk, q)
    S, mods, roots = R.s_ext(sk, q, psi)
    E = round2_errors(seed, N, dn)
    En = np.stack([np.stack([_ntt_small(E[v, j], mods, roots) for j in range(dn)]) for v in range(2)])
    return En, S, mods


def round2_from_terms(terms, joint):
    """round2(seed, joint, sk, q, psi) from round2_terms(seed, sk, q, psi)."""
    En, S, mods = terms
    joint = np.asarray(joint, np.uint64)
    out = np.empty_like(joint)
    for t, mt in enumerate(mods):
        m = np.uint64(mt)
        out[:, :, t] = (R.mulmod(joint[:, :, t], S[t], m) + En[:, :, t]) % m
    return out


def first_index_with_galois_above(N, bound):
    """The smallest r > 0 with 5^r mod 2N > bound."""
    r, g = 1, 5 % (2 * N)
    while g <= bound:
        r, g = r + 1, (g * 5) % (2 * N)
    return r
