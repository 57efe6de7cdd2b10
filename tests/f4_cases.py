"""Operands and exact checks shared by tests/test_oracle_f4_levels.py (CPU) and
tests/test_gpu_f4_levels.py (MI355X): plain numpy, Python integers and the oracle.

EvalMult and ModReduce take raw [K][2][Ll][N] residues at any level, so the operands here
need not be ciphertexts: uniform residues, residues at the edges of their range, and
polynomials planted so that a known coefficient reaches ModUp or the centred lift.
"""
import numpy as np

import oracle as O

# Relinearization identity: out0 + out1 s - (c0 + c1 s + c2 s^2) is the key-switching error,
# and  |d| <= dnum alpha N B_e + kP (1 + N)  coefficient-wise:
#   sum over digits of D_j e_j / P with |D_j| < alpha Q_j (the fast basis conversion's
#   overshoot), Q_j <= P and |e_j| <= B_e < 2^6 (test_oracle_f4.test_evaluation_key_relation)
#   gives dnum alpha N B_e; ModDown's own conversion overshoots by < kP in each of u0 and u1 s
#   (|s| <= 1, N terms).  Below 2^22 for every chain tested (dnum 3, alpha 4, N 2^13), while
#   one wrong residue makes d uniform modulo Q_l >= 2^45.
DEFECT_CAP = 1 << 24


def _obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


def _residue_batch(rng, q, K, Ll, N):
    """[K][2][Ll][N] residues, uniform below each tower's modulus."""
    out = np.empty((K, 2, Ll, N), np.uint64)
    for t in range(Ll):
        out[:, :, t] = rng.integers(0, int(q[t]), size=(K, 2, N), dtype=np.uint64)
    return out


def _full_batch(q, K, Ll, N, poly0=None, poly1=None):
    """[K][2][Ll][N] with every residue q_t - 1, or 0 where poly0 / poly1 is 0."""
    out = np.empty((K, 2, Ll, N), np.uint64)
    for t in range(Ll):
        out[:, 0, t] = 0 if poly0 == 0 else int(q[t]) - 1
        out[:, 1, t] = 0 if poly1 == 0 else int(q[t]) - 1
    return out


def _planted_c2(rng, q, psi, Ll, alpha, N):
    """One operand pair (a, b), each [2][Ll][N], whose c2 = a1 b1 has known coefficients c:
    a1 = NTT(c) and b1 = 1.  For every digit j (towers [j alpha, (j+1) alpha) of Q_l) c holds 0,
    1 and q_t - 1 in all of the digit's towers at once, i.e. the digit's values 0, 1 and
    Q_j - 1, at 8 positions each; 8 more positions hold q_t - 1 in every tower (all digits at
    Q_j - 1 together); everything else is uniform.  -> (a, b, c [Ll][N])"""
    dn = -(-Ll // alpha)
    c = _residue_batch(rng, q, 1, Ll, N)[0, 0]
    pos = rng.permutation(N)[:8 * (3 * dn + 1)].reshape(3 * dn + 1, 8)
    for j in range(dn):
        for t in range(j * alpha, min(Ll, (j + 1) * alpha)):
            c[t, pos[3 * j]] = 0
            c[t, pos[3 * j + 1]] = 1
            c[t, pos[3 * j + 2]] = int(q[t]) - 1
    for t in range(Ll):
        c[t, pos[3 * dn]] = int(q[t]) - 1
    a = _residue_batch(rng, q, 1, Ll, N)[0]
    b = _residue_batch(rng, q, 1, Ll, N)[0]
    for t in range(Ll):
        a[1, t] = O.ntt_fwd(c[t], int(q[t]), int(psi[t]))
    b[1] = 1
    return a, b, c


def _edge_batch(rng, q, psi, Ll, alpha, N, K):
    """The "edges" operand class -> (a, b), each [K][2][Ll][N].  K = 3: both operands all
    q_t - 1; a = (all 0, all q_t - 1) against a uniform b; the planted c2.  K = 1: the planted
    c2 alone."""
    pa, pb, _ = _planted_c2(rng, q, psi, Ll, alpha, N)
    if K == 1:
        return pa[None].copy(), pb[None].copy()
    assert K == 3
    full = _full_batch(q, 1, Ll, N)
    a = np.concatenate([full, _full_batch(q, 1, Ll, N, poly0=0), pa[None]])
    b = np.concatenate([full, _residue_batch(rng, q, 1, Ll, N), pb[None]])
    return a, b


def _planted_rescale_input(rng, q, psi, Ll, N):
    """One ModReduce input [1][2][Ll][N] (EVALUATION) with known integer coefficients, and what
    ModReduce must return.  c = k q_l + r with h = (q_l - 1) / 2 and r in {0, 1, h, h + 1,
    q_l - 1} at 8 positions each per polynomial (k = 0, negative and positive among them),
    |c| < Q_l / 4, the rest uniform in that range.  The centred lift of the last tower takes
    r <= h as r and r > h as r - q_l, so the result is round(c / q_l) = floor((2c + q_l) /
    (2 q_l)) in every remaining tower (q_l is odd: no tie).
    -> (ct, exp [2][Ll-1][N] COEFFICIENT residues of the expected output)"""
    ql = int(q[Ll - 1])
    h = (ql - 1) // 2
    Q = 1
    for t in range(Ll):
        Q *= int(q[t])
    kmax = Q // (4 * ql) - 2  # |k q_l + r| < Q_l / 4
    wide = max(1, kmax.bit_length() - 1)

    def rand_k(n):  # uniform in [-2^wide, 2^wide) from 62-bit pieces
        v = np.zeros(n, dtype=object)
        for _ in range(-(-(wide + 1) // 62)):
            v = v * (1 << 62) + rng.integers(0, 1 << 62, size=n).astype(object)
        return list(v % (1 << (wide + 1)) - (1 << wide))

    ct = np.empty((1, 2, Ll, N), np.uint64)
    exp = np.empty((2, Ll - 1, N), np.uint64)
    for poly in range(2):
        k = rand_k(N)
        r = [int(v) for v in rng.integers(0, ql, size=N)]
        pos = rng.permutation(N)[:40].reshape(5, 8)
        for row, rv in zip(pos, (0, 1, h, h + 1, ql - 1)):
            for i, n in enumerate(row):
                r[n] = rv
                if i == 0:
                    k[n] = 0
                elif i == 1:
                    k[n] = -abs(k[n]) - 1
                elif i == 2:
                    k[n] = abs(k[n]) + 1
                elif i == 3:
                    k[n] = -1
        c = np.array([kk * ql + rr for kk, rr in zip(k, r)], dtype=object)
        assert max(abs(v) for v in c) < Q // 4
        for t in range(Ll):
            qt = int(q[t])
            ct[0, poly, t] = O.ntt_fwd(np.array(c % qt, dtype=np.uint64), qt, int(psi[t]))
        rounded = (2 * c + ql) // (2 * ql)
        for t in range(Ll - 1):
            exp[poly, t] = np.array(rounded % int(q[t]), dtype=np.uint64)
    return ct, exp


def _rescale_coeffs(out, q, psi):
    """COEFFICIENT residues of one ModReduce output [2][Lo][N]."""
    return np.stack([np.stack([O.ntt_inv(out[p, t], int(q[t]), int(psi[t])) for t in range(out.shape[1])])
                     for p in range(2)])


def _relin_defect(out, a, b, sk, q, psi):
    """max |d| over the batch, d = out0 + out1 s - (a0 b0 + (a0 b1 + a1 b0) s + a1 b1 s^2):
    per tower t < Ll in EVALUATION form with Python integers, then inverse NTT and the centred
    CRT value over Q_l.  out, a, b [K][2][Ll][N]; sk [>= Ll][N] (EVALUATION)."""
    K, _, Ll, N = out.shape
    qs = [int(v) for v in q[:Ll]]
    Q = 1
    for v in qs:
        Q *= v
    worst = 0
    for k in range(K):
        X = np.zeros(N, dtype=object)
        for t, qt in enumerate(qs):
            s = _obj(sk[t])
            o0, o1, a0, a1, b0, b1 = (_obj(v[k, p, t]) for v in (out, a, b) for p in range(2))
            d = (o0 + o1 * s - (a0 * b0 + (a0 * b1 + a1 * b0) % qt * s + a1 * b1 % qt * s % qt * s)) % qt
            dc = O.ntt_inv(np.array(d, dtype=np.uint64), qt, int(psi[t])).astype(object)
            Qh = Q // qt
            X = X + dc * pow(Qh % qt, -1, qt) % qt * Qh
        X = X % Q
        worst = max(worst, max(min(v, Q - v) for v in X))
    return int(worst)
