"""EvalInnerProduct without a device: the yardstick tests/test_gpu_dot.py measures the
kernels with (tests/dot_ref.py) checked for what it must mean.  At one pair it is the oracle's EvalMult; over
K encrypted vectors it decodes, after ModReduce, to sum_k x_k y_k; its one key switch satisfies the
relinearization identity on the summed tensor with a defect that does not grow with K; and the squared
form is the general form on a copy.  Shape: ring 2^11, 3 towers, 52-bit scale."""
import functools

import numpy as np
import pytest

import dot_ref as DR
import f4_cases as F
import oracle as O

N, L, SEED, S = 1 << 11, 3, 91, 1 << 10


@functools.lru_cache(maxsize=None)
def _keys():
    q, psi = O.params_generate(N, L, 52, 60)
    s, e, a = O.sample_keygen(SEED, N, q)
    sk, pk = O.keygen(s, e, a, q, psi)
    evk = O.evk_keygen(SEED, sk, q, psi)
    return q, psi, sk, pk, evk


@functools.lru_cache(maxsize=None)
def _vectors(K):
    """K ciphertext pairs of uniform [-1, 1] slot vectors, and the vectors."""
    q, psi, sk, pk, evk = _keys()
    rng = np.random.default_rng([K, 5])
    x, y = rng.uniform(-1, 1, K * S), rng.uniform(-1, 1, K * S)
    delta = float(q[-1])
    a = O.encrypt_vector(x, pk, q, psi, N, S, delta, SEED)
    b = O.encrypt_vector(y, pk, q, psi, N, S, delta, SEED, g0=K)
    return x.reshape(K, S), y.reshape(K, S), a, b


def test_one_pair_is_eval_mult():
    q, psi, sk, pk, evk = _keys()
    rng = np.random.default_rng(1)
    a, b = (F._residue_batch(rng, q, 1, L, N) for _ in range(2))
    assert np.array_equal(DR.dot_ref(a, b, evk, q, psi), O.eval_mult(a, b, evk, q, psi))
    a, b = F._edge_batch(rng, q, psi, L, 2, N, 1)
    assert np.array_equal(DR.dot_ref(a, b, evk, q, psi), O.eval_mult(a, b, evk, q, psi))


@pytest.mark.parametrize("K", [8, 17])
def test_decodes_to_the_inner_product(K):
    """A wrong residue anywhere makes the decoded value uniform modulo Q; the measured error is 1.2e-11 at
    K = 8 and 2.1e-11 at K = 17 (the per-ciphertext path's: 1.2e-11, 2.2e-11)."""
    q, psi, sk, pk, evk = _keys()
    x, y, a, b = _vectors(K)
    out = O.rescale(DR.dot_ref(a, b, evk, q, psi), q, psi)
    assert out.shape == (1, 2, L - 1, N)
    scale = float(q[-1]) * float(q[-1]) / float(q[L - 1])
    dec = O.decrypt_vector(out, sk[:L - 1], q[:L - 1], psi[:L - 1], S, scale, S)
    err = float(np.abs(dec - (x * y).sum(axis=0)).max())
    print("K = %d: max error %.3g" % (K, err))
    assert err < 1e-9


@pytest.mark.parametrize("K", [1, 8, 17])
def test_relinearization_identity_on_the_summed_tensor(K):
    """One key switch: the defect stays under f4_cases.DEFECT_CAP whatever K is."""
    q, psi, sk, pk, evk = _keys()
    rng = np.random.default_rng([K, 6])
    a, b = (F._residue_batch(rng, q, K, L, N) for _ in range(2))
    c0, c1, c2 = DR.tensor_sums(a, b, q)
    out = DR.relin_ref(c0, c1, c2, evk, q, psi)
    d = DR.relin_defect(out, c0, c1, c2, sk, q, psi)
    print("K = %d: max|d| = %d" % (K, d))
    assert d < F.DEFECT_CAP


def test_square_is_the_general_form_on_a_copy():
    q, psi, sk, pk, evk = _keys()
    a = F._residue_batch(np.random.default_rng(7), q, 5, L, N)
    assert np.array_equal(DR.dot_ref(a, a, evk, q, psi), DR.dot_ref(a, a.copy(), evk, q, psi))
    c0, c1, c2 = DR.tensor_sums(a, a, q)
    for t in range(L):  # c1 = 2 sum a0 a1
        m = np.uint64(q[t])
        s = np.zeros(N, np.uint64)
        for k in range(5):
            s = (s + DR.R.mulmod(a[k, 0, t], a[k, 1, t], m)) % m
        assert np.array_equal(c1[t], (s + s) % m)


def test_tensor_sums_against_python_integers():
    """The numpy sums against big-integer arithmetic on a few positions, maximal residues among them."""
    q = _keys()[0]
    rng = np.random.default_rng(8)
    a = np.concatenate([F._residue_batch(rng, q, 2, L, N), F._full_batch(q, 2, L, N)])
    b = np.concatenate([F._full_batch(q, 1, L, N), F._residue_batch(rng, q, 3, L, N)])
    c = DR.tensor_sums(a, b, q)
    for t in range(L):
        qt = int(q[t])
        for n in (0, 1, N // 2, N - 1):
            a0, a1, b0, b1 = ([int(v) for v in w[:, p, t, n]] for w in (a, b) for p in range(2))
            assert int(c[0][t, n]) == sum(u * v for u, v in zip(a0, b0)) % qt
            assert int(c[1][t, n]) == sum(u * w + v * z for u, v, z, w in zip(a0, a1, b0, b1)) % qt
            assert int(c[2][t, n]) == sum(u * v for u, v in zip(a1, b1)) % qt
