"""Numpy restatement of EvalInnerProduct(ct, pt): the yardstick tests/test_gpu_dot_plain.py
measures the kernels with, checked for meaning against the oracle alone in tests/test_dotp_ref.py.

Ciphertext batches are uint64 [K][2][l][N], plaintext batches uint64 [K][l][N], both EVALUATION with canonical
residues; tower t is over q[t].  Products go through rotation_ref.mulmod (four bits at a time in uint64) and
sums through uint64 additions of two canonical residues, each followed by its remainder -- exact integers
throughout, so nothing here shares a reduction with the device code; project_ints states single positions in
Python integers."""
import numpy as np

import oracle as O
import plain_ref as PR
import rotation_ref as R_


def project_ref(batches, pts, q):
    """out [C R][2][l][N], entry c R + r: sum_k batches[c][k] (.) pts[r][k] in both components.  pts: [R][K][l][N],
    or [K][l][N] for R = 1."""
    batches = [np.asarray(b, np.uint64) for b in batches]
    pts = np.asarray(pts, np.uint64)
    if pts.ndim == 3:
        pts = pts[None]
    K, _, l, N = batches[0].shape
    assert pts.ndim == 4 and pts.shape[1:] == (K, l, N)
    R = pts.shape[0]
    out = np.zeros((len(batches) * R, 2, l, N), np.uint64)
    for c, b in enumerate(batches):
        assert b.shape == (K, 2, l, N)
        for r in range(R):
            for t in range(l):
                qt = np.uint64(q[t])
                acc = out[c * R + r, :, t]
                for k in range(K):
                    # a canonical sum plus a canonical product stays below 2^61: the remainder is exact
                    acc[:] = (acc + R_.mulmod(b[k, :, t], pts[r, k, t][None], qt)) % qt
    return out


def project_ints(batches, pts, q, c, r, i, t, n):
    """Entry c R + r, component i, tower t, coefficient n in Python integers: what project_ref must hold there."""
    return sum(int(batches[c][k, i, t, n]) * int(pts[r][k, t, n]) for k in range(batches[c].shape[0])) % int(q[t])


def one_hots(P, N, slots, q, psi, l):
    """The plaintexts [P][l][N] of the one-hot slot vectors e_0 .. e_{P-1}, at scale q[l - 1]."""
    pts = np.empty((P, l, N), np.uint64)
    for p in range(P):
        e = np.zeros(slots)
        e[p] = 1.0
        pts[p] = O.encode(e, N, slots, float(q[l - 1]), q[:l], psi[:l])
    return pts


def pack_ref(cts, slots, q, psi):
    """device.pack_slots: sum_p cts[p] (.) e_p, then the oracle's ModReduce: [P][2][l][N] -> [1][2][l-1][N]."""
    cts = np.asarray(cts, np.uint64)
    P, _, l, N = cts.shape
    pts = one_hots(P, N, slots, q, psi, l)
    if P == 1:  # (one product: the plaintext-operand yardstick itself)
        assert np.array_equal(project_ref([cts], pts, q), PR.mult_plain(cts, pts, q))
    return O.rescale(project_ref([cts], pts, q), q[:l], psi[:l])
