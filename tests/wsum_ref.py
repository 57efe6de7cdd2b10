"""Reference for EvalLinearWSum with encrypted weights, built from tests/dot_ref.py and the
oracle only: for every output k the summed tensor over the LEARNER axis -- dot_ref.tensor_sums of the stacked
weights against the stacked k-th update ciphertexts, the updates' towers cut to the weights' -- and ONE batched
relinearization, O.eval_mult of the K ciphertexts (0, c2_k) by (0, 1), plus (c0_k, c1_k), as tests/gram_ref.py
does for its pairs.  The oracle's EvalMult treats the ciphertexts of a batch independently, so entry k is
dot_ref.dot_ref(weights, column k) (tests/test_wsum_ref.py checks that).

Test infrastructure only; nothing here is imported by the product."""
import numpy as np

import dot_ref as DR
import oracle as O


def columns(us, ws, k):
    """(W, U), each [C][2][l][N]: the learners' weights for output k and their k-th update ciphertexts, the
    updates' first l towers.  us: C arrays [K][2][lu][N]; ws: C arrays [Kw][2][l][N], Kw = 1 or K."""
    l = ws[0].shape[2]
    W = np.stack([w[k if w.shape[0] > 1 else 0] for w in ws])
    U = np.stack([u[k][:, :l] for u in us])
    return W, U


def tensor_sums(us, ws, q):
    """c [K][3][l][N]: for every k the sums over the learners of the three tensor components."""
    us, ws = [np.asarray(u, np.uint64) for u in us], [np.asarray(w, np.uint64) for w in ws]
    assert len(us) == len(ws) >= 1
    K, _, lu, N = us[0].shape
    Kw, _, l, _ = ws[0].shape
    assert Kw in (1, K) and l <= lu
    assert all(u.shape == us[0].shape for u in us) and all(w.shape == ws[0].shape for w in ws)
    c = np.zeros((K, 3, l, N), np.uint64)
    for k in range(K):
        c[k, 0], c[k, 1], c[k, 2] = DR.tensor_sums(*columns(us, ws, k), q)
    return c


def wsum_ref(us, ws, evk, q, psi):
    """[K][2][l][N]: entry k is EvalInnerProduct over the learners of (weight for k, k-th update); q / psi the
    whole chain."""
    c = tensor_sums(us, ws, q)
    K, _, l, N = c.shape
    X, Y = np.zeros((K, 2, l, N), np.uint64), np.zeros((K, 2, l, N), np.uint64)
    X[:, 1] = c[:, 2]
    Y[:, 1] = 1  # the constant 1 in EVALUATION
    out = O.eval_mult(X, Y, evk, q, psi)
    ql = np.asarray(q[:l], np.uint64)[None, None, :, None]
    return (out + c[:, :2]) % ql
