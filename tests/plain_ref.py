"""Numpy restatement of the plaintext-operand calls: the yardstick
tests/test_gpu_plain_ops.py measures the kernels with, checked for meaning against the oracle alone in
tests/test_plain_ref.py.

Ciphertexts are uint64 [K][2][l][N], plaintexts uint64 [Kp][l][N] with Kp = K or 1 (a [l][N] plaintext
counts as Kp = 1), both EVALUATION with canonical residues; tower t is over q[t].  Products go through
Python-int object arrays and sums through numpy's uint64 remainder (operands below 2^60 cannot wrap),
so nothing here shares a reduction with the device code."""
import numpy as np


def _q(q, l):
    return np.array([int(v) for v in q[:l]], dtype=object).reshape(1, l, 1)


def _pt(pt, K):
    pt = np.asarray(pt, np.uint64)
    if pt.ndim == 2:
        pt = pt[None]
    assert pt.ndim == 3 and pt.shape[0] in (1, K)
    return pt


def _obj(a):
    return np.asarray(a, np.uint64).astype(object)


def mult_plain(ct, pt, q):
    """cc->EvalMult(ct, pt): both components times the plaintext."""
    ct = np.asarray(ct, np.uint64)
    K, _, l, _ = ct.shape
    p, qq = _obj(_pt(pt, K)), _q(q, l)
    out = np.empty_like(ct)
    for c in range(2):
        out[:, c] = ((_obj(ct[:, c]) * p) % qq).astype(np.uint64)
    return out


def _qu(q, l):
    return np.asarray(q[:l], np.uint64).reshape(l, 1)


def _c0(ct, pt, q, add):
    ct = np.asarray(ct, np.uint64)
    K, _, l, _ = ct.shape
    qq, p = _qu(q, l), _pt(pt, K)
    out = ct.copy()
    # canonical operands below 2^60: a + p and a + (q - p) stay below 2^61 in uint64
    out[:, 0] = (ct[:, 0] + (p if add else qq - p)) % qq
    return out


def add_plain(ct, pt, q):
    """cc->EvalAdd(ct, pt): c0 + pt, c1 unchanged."""
    return _c0(ct, pt, q, True)


def sub_plain(ct, pt, q):
    """cc->EvalSub(ct, pt): c0 - pt, c1 unchanged."""
    return _c0(ct, pt, q, False)


def sub(a, b, q):
    """cc->EvalSub(a, b): a - b in every residue, in [0, q): a - a is 0."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    qq = _qu(q, a.shape[2])
    return (a + (qq - b)) % qq


def neg(a, q):
    """cc->EvalNegate(a): q - a, and 0 for 0."""
    a = np.asarray(a, np.uint64)
    qq = _qu(q, a.shape[2])
    return (qq - a) % qq


SPAN = 8  # planted coefficients at either end of a polynomial


def plant(buf, q, values, div=1):
    """Edge residues in the first SPAN coefficients (coefficient 0 first) and, mirrored, the last SPAN
    (coefficient N - 1 first) of every polynomial of buf [..., l, N] (in place; returned): position j
    takes values[(j // div) % len(values)](q_t).  A plaintext planted with PT_EDGES and a ciphertext
    with CT_EDGES at div = 4 meet in all 8 combinations at either end, (q - 1)(q - 1) among them."""
    l, N = buf.shape[-2], buf.shape[-1]
    for t in range(l):
        qt = int(q[t])
        for j in range(SPAN):
            v = values[(j // div) % len(values)](qt)
            buf[..., t, j] = v
            buf[..., t, N - 1 - j] = v
    return buf


PT_EDGES = (lambda q: q - 1, lambda q: 0, lambda q: 1, lambda q: q - 2)
CT_EDGES = (lambda q: q - 1, lambda q: 0)
