"""EvalInnerProduct(ct, pt) without a device: the yardstick tests/test_gpu_dot_plain.py measures
the kernels with (tests/dotp_ref.py) checked for what it must mean, against the oracle and tests/plain_ref.py
alone.  At one ciphertext it is mult_plain; over K it is the exact modular sum of the K mult_plain products; on
encrypted vectors against encoded ones it decodes, after ModReduce and a sum over slots, to sum x g; and pack_ref
puts slot p of ciphertext p into slot p of one ciphertext.  Shape: ring 2^11, 3 towers, 52-bit scale."""
import functools

import numpy as np
import pytest

import dotp_ref as PJ
import f4_cases as F
import oracle as O
import plain_ref as PR

N, L, SEED, S = 1 << 11, 3, 93, 1 << 10


@functools.lru_cache(maxsize=None)
def _keys(L=L):
    q, psi = O.params_generate(N, L, 52, 60)
    s, e, a = O.sample_keygen(SEED, N, q)
    sk, pk = O.keygen(s, e, a, q, psi)
    return q, psi, sk, pk


def _plain_batch(rng, q, K, l):
    return F._residue_batch(rng, q, K, l, N)[:, 0].copy()


def test_one_ciphertext_is_mult_plain():
    q = _keys()[0]
    rng = np.random.default_rng(1)
    ct, pt = F._residue_batch(rng, q, 1, L, N), _plain_batch(rng, q, 1, L)
    PR.plant(ct, q, PR.CT_EDGES, div=4)
    PR.plant(pt, q, PR.PT_EDGES)
    assert np.array_equal(PJ.project_ref([ct], pt, q), PR.mult_plain(ct, pt, q))
    assert np.array_equal(PJ.project_ref([ct], pt[None], q), PR.mult_plain(ct, pt, q))


@pytest.mark.parametrize("K", [8, 17])
def test_k_ciphertexts_are_the_sum_of_k_mult_plains(K):
    q = _keys()[0]
    rng = np.random.default_rng([K, 2])
    cts = [F._residue_batch(rng, q, K, L, N) for _ in range(2)]
    pts = np.stack([_plain_batch(rng, q, K, L) for _ in range(3)])
    PR.plant(cts[1], q, PR.CT_EDGES, div=4)
    PR.plant(pts[2], q, PR.PT_EDGES)
    got = PJ.project_ref(cts, pts, q)
    assert got.shape == (6, 2, L, N)
    qq = np.asarray(q[:L], np.uint64).reshape(1, L, 1)
    for c in range(2):
        for r in range(3):
            prod = PR.mult_plain(cts[c], pts[r], q)  # [K][2][L][N], each below q < 2^60
            acc = np.zeros((2, L, N), np.uint64)
            for k in range(K):
                acc = (acc + prod[k]) % qq
            assert np.array_equal(got[c * 3 + r], acc), (c, r)
    # and single positions in Python integers, the planted maximal residues among them
    for c, r, i, t, n in ((0, 0, 0, 0, 0), (1, 2, 1, 0, 0), (1, 2, 0, 2, N - 1), (1, 1, 1, 1, N // 2), (0, 2, 0, 1, 5)):
        assert int(got[c * 3 + r, i, t, n]) == PJ.project_ints(cts, pts, q, c, r, i, t, n)


@pytest.mark.parametrize("K", [8, 17])
def test_decodes_to_the_inner_product(K):
    """Encrypted U(-1, 1) vectors against encoded U(-1, 1) vectors at scale q_{l-1}: after ModReduce, decrypt and
    the sum over slots the value is sum x g.  A wrong residue anywhere makes the decoded value uniform modulo Q;
    the measured error is 4.5e-11 at K = 8 and 3.2e-11 at K = 17."""
    q, psi, sk, pk = _keys()
    rng = np.random.default_rng([K, 3])
    x, g = rng.uniform(-1, 1, (K, S)), rng.uniform(-1, 1, (K, S))
    delta = float(q[-1])
    ct = O.encrypt_vector(x.reshape(-1), pk, q, psi, N, S, delta, SEED)
    pt = np.stack([O.encode(v, N, S, float(q[L - 1]), q, psi) for v in g])
    out = O.rescale(PJ.project_ref([ct], pt, q), q, psi)
    assert out.shape == (1, 2, L - 1, N)
    scale = delta * float(q[L - 1]) / float(q[L - 1])
    dec = O.decrypt_vector(out, sk[:L - 1], q[:L - 1], psi[:L - 1], S, scale, S)
    err = abs(float(dec.sum()) - float((x * g).sum()))
    print("K = %d: error %.3g" % (K, err))
    assert err < 1e-9


def test_pack_ref_puts_each_constant_in_its_slot():
    """P = 5 ciphertexts of distinct constants on a 4-tower chain, one ModReduce already spent: the packed
    ciphertext ends on 2 towers and decodes to the constants in slots 0..4 and to nothing elsewhere."""
    q, psi, sk, pk = _keys(4)
    delta = float(q[-1])
    consts = np.array([0.75, -1.5, 3.25, 0.001, -100.0])
    cts = O.encrypt_vector(np.repeat(consts, S), pk, q, psi, N, S, delta, SEED)
    assert cts.shape == (5, 2, 4, N)
    low = cts[:, :, :3].copy()  # the same ciphertexts at 3 towers: dropping a tower keeps the message
    out = PJ.pack_ref(low, S, q, psi)
    assert out.shape == (1, 2, 2, N)
    dec = O.decrypt_vector(out, sk[:2], q[:2], psi[:2], S, delta, S)
    err = float(np.abs(dec[:5] - consts).max())
    rest = float(np.abs(dec[5:]).max())
    print("pack_ref: slots 0..4 off by %.3g, the rest at most %.3g" % (err, rest))
    assert err < 1e-6 and rest < 1e-6
