"""Reference for hoisted rotations: decompose, inner product and ModDown restated in numpy
over the oracle's ntt_fwd / ntt_inv / special_primes and rotation_ref's mulmod / gather_index.

  decompose(c1)      D_j, j < dn: digit j of c1 over Q_l u P in EVALUATION -- the digit's own towers are c1's
                     residues, the foreign ones NTT(ModUp_j(INTT(c1))), or_eval_mult's arithmetic
  inner(D, g, key)   U = sum_j sigma_g(D_j) (.) (b_j, a_j) over every tower of Q_l u P; sigma_g the gather
                     out[p] = in[gather_index(N, g)[p]]
  mod_down(U)        (U_Q - NTT(Conv_{P -> Q_l}(INTT(U_P)))) P^-1
  hoisted_ref        out_r = (sigma_{g_r}(c0), 0) + mod_down(inner(decompose(c1), g_r, key_r))

With g = 1 this is O.eval_mult((0, c), (0, 1), key) bit for bit (tests/test_hoist_ref.py), which ties every
constant and the tower order to the oracle.  It is NOT rotation_ref.rotate_ref: that decomposes sigma_g(c1).

Test infrastructure only; nothing here is imported by the product."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle as O
import rotation_ref as R


def basis(q, l, N):
    """-> (dn, alpha, mods, roots, kP) of Q_l u P for ciphertexts of l towers of the chain q."""
    _, al, p, pr = O.special_primes(N, q)
    return (l + al - 1) // al, al, [int(v) for v in p], [int(v) for v in pr]


def decompose(c1, q, psi):
    """c1 [l][N] (EVALUATION) -> D [dn][l + kP][N] (EVALUATION over Q_l u P)."""
    c1 = np.asarray(c1, np.uint64)
    l, N = c1.shape
    dn, al, p, pr = basis(q, l, N)
    mods = [int(v) for v in q[:l]] + p
    roots = [int(v) for v in psi[:l]] + pr
    T = len(mods)
    coef = np.stack([O.ntt_inv(c1[t], mods[t], roots[t]) for t in range(l)])
    D = np.zeros((dn, T, N), np.uint64)
    for j in range(dn):
        s0 = j * al
        own = range(s0, min(s0 + al, l))
        # y_i = [c_i (Q_j / q_i)^-1]_{q_i}
        y = {}
        for i in own:
            qi, h = mods[i], 1
            for v in own:
                if v != i:
                    h = h * (mods[v] % qi) % qi
            y[i] = R.mulmod(coef[i], np.uint64(pow(h, -1, qi)), qi)
        for t in range(T):
            if t in own:
                D[j, t] = c1[t]
                continue
            mt = mods[t]
            acc = np.zeros(N, np.uint64)
            for i in own:
                h = 1
                for v in own:
                    if v != i:
                        h = h * (mods[v] % mt) % mt
                acc = (acc + R.mulmod(y[i] % np.uint64(mt), np.uint64(h), mt)) % np.uint64(mt)
            D[j, t] = O.ntt_fwd(acc, mt, roots[t])
    return D


def inner(D, g, key, q):
    """U [2][T][N] = sum_j sigma_g(D_j) (.) (key[0][j], key[1][j]); key [2][dnum][L + kP][N]."""
    dn, T, N = D.shape
    L = len(q)
    kP = np.asarray(key).shape[2] - L
    l = T - kP
    _, _, p, _ = basis(q, l, N)
    mods = [int(v) for v in q[:l]] + p
    src = R.gather_index(N, g)
    U = np.zeros((2, T, N), np.uint64)
    for t in range(T):
        tk = t if t < l else L + (t - l)  # the key's tower
        m = np.uint64(mods[t])
        for j in range(dn):
            d = D[j, t][src]
            for c in range(2):
                U[c, t] = (U[c, t] + R.mulmod(d, key[c][j][tk], m)) % m
    return U


def mod_down(U, q, psi):
    """U [2][l + kP][N] (EVALUATION) -> [2][l][N]."""
    U = np.asarray(U, np.uint64)
    _, T, N = U.shape
    _, _, p, pr = O.special_primes(N, q)
    p, pr = [int(v) for v in p], [int(v) for v in pr]
    kP = len(p)
    l = T - kP
    out = np.zeros((2, l, N), np.uint64)
    for c in range(2):
        y = []
        for m in range(kP):
            h = 1
            for v in range(kP):
                if v != m:
                    h = h * (p[v] % p[m]) % p[m]
            y.append(R.mulmod(O.ntt_inv(U[c, l + m], p[m], pr[m]), np.uint64(pow(h, -1, p[m])), p[m]))
        for t in range(l):
            qt = int(q[t])
            acc = np.zeros(N, np.uint64)
            P = 1
            for m in range(kP):
                P = P * (p[m] % qt) % qt
                h = 1
                for v in range(kP):
                    if v != m:
                        h = h * (p[v] % qt) % qt
                acc = (acc + R.mulmod(y[m] % np.uint64(qt), np.uint64(h), qt)) % np.uint64(qt)
            z = O.ntt_fwd(acc, qt, int(psi[t]))
            diff = (U[c, t] + np.uint64(qt) - z) % np.uint64(qt)
            out[c, t] = R.mulmod(diff, np.uint64(pow(P, -1, qt)), qt)
    return out


def key_switch_hoisted(D, g, key, q, psi):
    """ModDown(sum_j sigma_g(D_j) (.) key_j): [2][l][N]."""
    return mod_down(inner(D, g, key, q), q, psi)


def hoisted_ref(ct, rs, keys, q, psi):
    """rotate_many(ct, rs): ct [K][2][l][N]; keys {index: key [2][dnum][L + kP][N]} (index 0 needs none);
    -> [R][K][2][l][N]."""
    ct = np.asarray(ct, np.uint64)
    K, _, l, N = ct.shape
    ql = np.asarray(q[:l], np.uint64)[:, None]
    rs = [int(r) for r in rs]

    def one(k):
        D = decompose(ct[k, 1], q, psi) if any(rs) else None
        done = {}
        for r in rs:
            if r in done:
                continue
            if not r:
                done[r] = ct[k].copy()
                continue
            g = R.galois(N, r)
            o = key_switch_hoisted(D, g, keys[r], q, psi)
            o[0] = (o[0] + ct[k, 0][:, R.gather_index(N, g)]) % ql
            done[r] = o
        return np.stack([done[r] for r in rs])

    with ThreadPoolExecutor(max_workers=max(1, min(K, 8))) as pool:
        outs = list(pool.map(one, range(K)))
    return np.stack(outs, axis=1)
