"""Reference for the Gram matrix of encrypted batches, built from tests/dot_ref.py and the
oracle only: the summed tensor of every pair (i, j), i <= j, and ONE batched relinearization -- O.eval_mult of
the P ciphertexts (0, c2_p) by (0, 1), the device dot_ref.relin_ref uses with one ciphertext -- plus (c0_p,
c1_p).  The oracle's EvalMult treats the ciphertexts of a batch independently, so entry p is
dot_ref.dot_ref(u_i, u_j) (tests/test_gram_ref.py checks that).

Test infrastructure only; nothing here is imported by the product."""
import numpy as np

import dot_ref as DR
import oracle as O


def pair_index(i, j, C):
    """Index of the pair (i, j), i <= j < C: the upper triangle, row-major."""
    assert 0 <= i <= j < C
    return i * C - i * (i - 1) // 2 + (j - i)


def pairs(C):
    """The pairs in output order: pairs(C)[pair_index(i, j, C)] == (i, j)."""
    return [(i, j) for i in range(C) for j in range(i, C)]


def gram_ref(batches, evk, q, psi):
    """[P][2][l][N], P = C (C + 1) / 2: entry pair_index(i, j, C) is EvalInnerProduct(batches[i], batches[j]).
    batches: C arrays [K][2][l][N] (EVALUATION, canonical residues); q / psi the whole chain."""
    batches = [np.asarray(b, np.uint64) for b in batches]
    C = len(batches)
    K, _, l, N = batches[0].shape
    P = C * (C + 1) // 2
    X, Y = np.zeros((P, 2, l, N), np.uint64), np.zeros((P, 2, l, N), np.uint64)
    c01 = np.zeros((P, 2, l, N), np.uint64)
    Y[:, 1] = 1  # the constant 1 in EVALUATION
    for p, (i, j) in enumerate(pairs(C)):
        c01[p, 0], c01[p, 1], X[p, 1] = DR.tensor_sums(batches[i], batches[j], q)
    out = O.eval_mult(X, Y, evk, q, psi)
    ql = np.asarray(q[:l], np.uint64)[None, None, :, None]
    return (out + c01) % ql
