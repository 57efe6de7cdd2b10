"""The Gram matrix without a device: the yardstick tests/test_gpu_gram.py measures the
kernels with (tests/gram_ref.py) checked for what it must mean.  Its pair order is the closed form of
include/shelfi.h; at one ciphertext a batch it is the oracle's EvalMult on the three pairs; every entry is
dot_ref's EvalInnerProduct of its pair; and over encrypted vectors the entries decode, after ModReduce, to
sum_k x_ik x_jk.  Shape: ring 2^11, 3 towers, 52-bit scale."""
import functools

import numpy as np

import dot_ref as DR
import f4_cases as F
import gram_ref as GR
import oracle as O

N, L, SEED, S = 1 << 11, 3, 93, 1 << 10


@functools.lru_cache(maxsize=None)
def _keys():
    q, psi = O.params_generate(N, L, 52, 60)
    s, e, a = O.sample_keygen(SEED, N, q)
    sk, pk = O.keygen(s, e, a, q, psi)
    evk = O.evk_keygen(SEED, sk, q, psi)
    return q, psi, sk, pk, evk


@functools.lru_cache(maxsize=None)
def _encrypted(C, K):
    """C batches of K ciphertexts of uniform [-1, 1] slot vectors, the vectors [C][K][S], and their Gram
    reference (computed once for the tests that read it)."""
    q, psi, sk, pk, evk = _keys()
    x = np.random.default_rng([C, K, 5]).uniform(-1, 1, (C, K, S))
    delta = float(q[-1])
    u = [O.encrypt_vector(x[i].reshape(-1), pk, q, psi, N, S, delta, SEED, g0=i * K) for i in range(C)]
    return x, u, GR.gram_ref(u, evk, q, psi)


def test_pairs_are_a_bijection_in_closed_form():
    for C in range(1, 33):
        ps = GR.pairs(C)
        assert len(ps) == C * (C + 1) // 2 == len(set(ps))
        assert [GR.pair_index(i, j, C) for i, j in ps] == list(range(len(ps)))
        assert all(0 <= i <= j < C for i, j in ps)
    assert GR.pairs(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def test_one_ciphertext_a_batch_is_eval_mult_on_the_three_pairs():
    q, psi, sk, pk, evk = _keys()
    rng = np.random.default_rng(1)
    for a, b in ([F._residue_batch(rng, q, 1, L, N) for _ in range(2)], F._edge_batch(rng, q, psi, L, 2, N, 1)):
        g = GR.gram_ref([a, b], evk, q, psi)
        assert g.shape == (3, 2, L, N)
        for p, (x, y) in enumerate(((a, a), (a, b), (b, b))):
            assert np.array_equal(g[p:p + 1], O.eval_mult(x, y, evk, q, psi)), p


def test_every_entry_is_the_inner_product_of_its_pair():
    q, psi, sk, pk, evk = _keys()
    rng = np.random.default_rng(2)
    u = [F._residue_batch(rng, q, 4, L, N) for _ in range(3)]
    g = GR.gram_ref(u, evk, q, psi)
    assert g.shape == (6, 2, L, N)
    for p, (i, j) in enumerate(GR.pairs(3)):
        assert np.array_equal(g[p:p + 1], DR.dot_ref(u[i], u[j], evk, q, psi)), (i, j)
    x, enc, ge = _encrypted(3, 4)
    for p, (i, j) in enumerate(GR.pairs(3)):
        assert np.array_equal(ge[p:p + 1], DR.dot_ref(enc[i], enc[j], evk, q, psi)), (i, j)


def test_entries_decode_to_the_inner_products():
    """A wrong residue anywhere makes a decoded value uniform modulo Q; test_dot_ref.py's bound."""
    q, psi, sk, pk, evk = _keys()
    x, enc, g = _encrypted(3, 4)
    out = O.rescale(g, q, psi)
    assert out.shape == (6, 2, L - 1, N)
    scale = float(q[-1]) * float(q[-1]) / float(q[L - 1])
    dec = O.decrypt_vector(out, sk[:L - 1], q[:L - 1], psi[:L - 1], S, scale, 6 * S).reshape(6, S)
    for p, (i, j) in enumerate(GR.pairs(3)):
        err = float(np.abs(dec[p] - (x[i] * x[j]).sum(axis=0)).max())
        print("pair (%d, %d): max error %.3g" % (i, j, err))
        assert err < 1e-9
