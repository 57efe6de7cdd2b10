"""Reference for EvalInnerProduct, built from the oracle's parts only: the summed
three-component tensor with tests/rotation_ref.py's mulmod, and the one relinearization as O.eval_mult of
(0, c2) by (0, 1) -- its tensor terms c0, c1 vanish and its c2 is ours, so it returns exactly
KeySwitch(c2) under the evaluation key (the device tests/rotation_ref.py's rotate_ref uses).

Test infrastructure only; nothing here is imported by the product."""
import numpy as np

import oracle as O
import rotation_ref as R


def tensor_sums(a, b, q):
    """(c0, c1, c2), each [l][N]: sum_k a_k0 b_k0, sum_k (a_k0 b_k1 + a_k1 b_k0), sum_k a_k1 b_k1 mod q_t
    over a, b [K][2][l][N] (EVALUATION, canonical residues)."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    K, _, l, N = a.shape
    assert b.shape == a.shape and K >= 1
    c = np.zeros((3, l, N), np.uint64)
    for t in range(l):
        m = np.uint64(q[t])
        a0, a1, b0, b1 = a[:, 0, t], a[:, 1, t], b[:, 0, t], b[:, 1, t]  # [K][N]
        p0, p2 = R.mulmod(a0, b0, m), R.mulmod(a1, b1, m)
        p1 = (R.mulmod(a0, b1, m) + R.mulmod(a1, b0, m)) % m
        for k in range(K):  # residues below 2^60: a sum of two never wraps
            c[0, t] = (c[0, t] + p0[k]) % m
            c[1, t] = (c[1, t] + p1[k]) % m
            c[2, t] = (c[2, t] + p2[k]) % m
    return c[0], c[1], c[2]


def relin_ref(c0, c1, c2, evk, q, psi):
    """(c0, c1) + KeySwitch(c2) under evk -> [1][2][l][N]; q / psi the whole chain."""
    c0, c1, c2 = (np.asarray(v, np.uint64) for v in (c0, c1, c2))
    l, N = c2.shape
    X, Y = np.zeros((1, 2, l, N), np.uint64), np.zeros((1, 2, l, N), np.uint64)
    X[0, 1] = c2
    Y[0, 1] = 1  # the constant 1 in EVALUATION
    out = O.eval_mult(X, Y, evk, q, psi)
    ql = np.asarray(q[:l], np.uint64)[:, None]
    out[0, 0] = (out[0, 0] + c0) % ql
    out[0, 1] = (out[0, 1] + c1) % ql
    return out


def relin_defect(out, c0, c1, c2, sk, q, psi):
    """max |d|, d = out0 + out1 s - (c0 + c1 s + c2 s^2): tests/f4_cases.py's _relin_defect on a summed
    tensor.  Per tower in EVALUATION with Python integers, then inverse NTT and the centred CRT value
    over Q_l.  out [1][2][l][N]; c0, c1, c2 [l][N]; sk [>= l][N] (EVALUATION)."""
    l, N = np.asarray(c2).shape
    qs = [int(v) for v in q[:l]]
    Q = 1
    for v in qs:
        Q *= v
    X = np.zeros(N, dtype=object)
    for t, qt in enumerate(qs):
        s, o0, o1, x0, x1, x2 = (np.asarray(v, np.uint64).astype(object)
                                 for v in (sk[t], out[0, 0, t], out[0, 1, t], c0[t], c1[t], c2[t]))
        d = (o0 + o1 * s - (x0 + x1 * s + x2 * s % qt * s)) % qt
        dc = O.ntt_inv(np.array(d, dtype=np.uint64), qt, int(psi[t])).astype(object)
        Qh = Q // qt
        X = X + dc * pow(Qh % qt, -1, qt) % qt * Qh
    X = X % Q
    return int(max(min(v, Q - v) for v in X))


def dot_ref(a, b, evk, q, psi):
    """EvalInnerProduct(a, b) at the operands' level: one relinearization of the summed tensor."""
    return relin_ref(*tensor_sums(a, b, q), evk, q, psi)
