"""EvalLinearWSum with encrypted weights without a device: the yardstick
tests/test_gpu_wsum_ct.py measures the kernel with (tests/wsum_ref.py) checked for what it must mean, with one
weight ciphertext a learner (Kw = 1) and with one per update ciphertext (Kw = K).  Every entry is dot_ref's
EvalInnerProduct of the stacked weights against the stacked k-th column; with one learner it is the oracle's
EvalMult; its one key switch per output satisfies the relinearization identity on the summed tensor; updates
stored at a higher level give what their prefix copies give; and over encrypted vectors the entries decode,
after ModReduce, to sum_c w_c x_c.  Shape: ring 2^11, 3 towers, 52-bit scale."""
import functools

import numpy as np
import pytest

import dot_ref as DR
import f4_cases as F
import oracle as O
import wsum_ref as WR

N, L, SEED, S = 1 << 11, 3, 97, 1 << 10


@functools.lru_cache(maxsize=None)
def _keys():
    q, psi = O.params_generate(N, L, 52, 60)
    s, e, a = O.sample_keygen(SEED, N, q)
    sk, pk = O.keygen(s, e, a, q, psi)
    evk = O.evk_keygen(SEED, sk, q, psi)
    return q, psi, sk, pk, evk


def _operands(C, K, Kw, seed, l=L, lu=L):
    q = _keys()[0]
    rng = np.random.default_rng([C, K, Kw, seed])
    return ([F._residue_batch(rng, q, K, lu, N) for _ in range(C)],
            [F._residue_batch(rng, q, Kw, l, N) for _ in range(C)])


@pytest.mark.parametrize("per_k", [False, True], ids=["Kw=1", "Kw=K"])
def test_every_entry_is_the_inner_product_of_its_column(per_k):
    q, psi, sk, pk, evk = _keys()
    C, K = 3, 4
    us, ws = _operands(C, K, K if per_k else 1, 1)
    r = WR.wsum_ref(us, ws, evk, q, psi)
    assert r.shape == (K, 2, L, N)
    for k in range(K):
        W = np.stack([w[k if per_k else 0] for w in ws])
        U = np.stack([u[k] for u in us])
        assert np.array_equal(r[k:k + 1], DR.dot_ref(W, U, evk, q, psi)), k


@pytest.mark.parametrize("per_k", [False, True], ids=["Kw=1", "Kw=K"])
def test_one_learner_is_eval_mult(per_k):
    q, psi, sk, pk, evk = _keys()
    K = 3
    us, ws = _operands(1, K, K if per_k else 1, 2)
    w = ws[0] if per_k else np.repeat(ws[0], K, axis=0)
    assert np.array_equal(WR.wsum_ref(us, ws, evk, q, psi), O.eval_mult(w, us[0], evk, q, psi))
    a, b = F._edge_batch(np.random.default_rng(3), q, psi, L, 2, N, 3)  # maximal residues and a planted c2
    assert np.array_equal(WR.wsum_ref([b], [a], evk, q, psi), O.eval_mult(a, b, evk, q, psi))


@pytest.mark.parametrize("per_k", [False, True], ids=["Kw=1", "Kw=K"])
@pytest.mark.parametrize("C", [1, 5])
def test_relinearization_identity_on_every_summed_tensor(C, per_k):
    """One key switch an output: the defect stays under f4_cases.DEFECT_CAP whatever C is."""
    q, psi, sk, pk, evk = _keys()
    K = 2
    us, ws = _operands(C, K, K if per_k else 1, 4)
    c = WR.tensor_sums(us, ws, q)
    r = WR.wsum_ref(us, ws, evk, q, psi)
    for k in range(K):
        d = DR.relin_defect(r[k:k + 1], c[k, 0], c[k, 1], c[k, 2], sk, q, psi)
        print("C = %d, k = %d: max|d| = %d" % (C, k, d))
        assert d < F.DEFECT_CAP


@pytest.mark.parametrize("per_k", [False, True], ids=["Kw=1", "Kw=K"])
def test_updates_at_a_higher_level_are_their_prefix(per_k):
    q, psi, sk, pk, evk = _keys()
    C, K = 2, 2
    us, ws = _operands(C, K, K if per_k else 1, 5, l=2, lu=3)
    r = WR.wsum_ref(us, ws, evk, q, psi)
    assert r.shape == (K, 2, 2, N)
    assert np.array_equal(r, WR.wsum_ref([np.ascontiguousarray(u[:, :, :2]) for u in us], ws, evk, q, psi))


@pytest.mark.parametrize("per_k", [False, True], ids=["Kw=1", "Kw=K"])
def test_entries_decode_to_the_weighted_sum(per_k):
    """A wrong residue anywhere makes a decoded value uniform modulo Q; test_dot_ref.py's bound (its sums are
    longer than these three terms)."""
    q, psi, sk, pk, evk = _keys()
    C, K = 3, 2
    Kw = K if per_k else 1
    rng = np.random.default_rng([6, Kw])
    x = rng.uniform(-1, 1, (C, K, S))
    wv = rng.uniform(0, 1, (C, Kw, S))
    wv[:, 0] = wv[:, 0, :1]  # a constant in every slot: a scalar weight; with Kw = K the second is per slot
    delta = float(q[-1])
    us = [O.encrypt_vector(x[i].reshape(-1), pk, q, psi, N, S, delta, SEED, g0=i * K) for i in range(C)]
    ws = [O.encrypt_vector(wv[i].reshape(-1), pk, q, psi, N, S, delta, SEED, g0=C * K + i * Kw) for i in range(C)]
    out = O.rescale(WR.wsum_ref(us, ws, evk, q, psi), q, psi)
    assert out.shape == (K, 2, L - 1, N)
    scale = delta * delta / float(q[L - 1])
    dec = O.decrypt_vector(out, sk[:L - 1], q[:L - 1], psi[:L - 1], S, scale, K * S).reshape(K, S)
    exp = (wv * x).sum(axis=0) if per_k else (wv[:, :1] * x).sum(axis=0)
    err = float(np.abs(dec - exp).max())
    print("max error %.3g" % err)
    assert err < 1e-9
