"""Hoisted rotations without a device: the yardstick tests/test_gpu_rotate_many.py measures
the kernels with (tests/hoist_ref.py) held to the oracle and to its meaning.

  to the oracle    with g = 1 the hoisted key switch of c under ANY key is O.eval_mult((0, c), (0, 1), key), bit
                   for bit: the tensor's c0, c1 vanish and c2 = c.  One, two and three digits (the last one
                   partial, kP = 3), and at truncated levels.
  to its meaning   under rotation keys (rotation_ref.rot_key_from_evk) hoisted_ref decrypts to the rolled slots
                   within tests/test_gpu_rotate.py's rule, max(1e-7, 2^(18 - scaleBits)).
  not rotate       hoisted_ref and rotation_ref.rotate_ref differ as residues: rotate decomposes sigma_g(c1),
                   and the approximate basis conversion does not commute with sigma_g's sign flips."""
import functools

import numpy as np
import pytest

import hoist_ref as H
import oracle as O
import rotation_ref as R
from f4_cases import _residue_batch

SEED = 91
# id: (ring, towers, (dnum, alpha, kP), levels)
CHAINS = {
    "one_digit": (1 << 11, 1, (1, 1, 1), (1,)),
    "two_digits": (1 << 11, 3, (2, 2, 2), (3, 2, 1)),       # level 3: a partial last digit
    "three_digits": (1 << 11, 7, (3, 3, 3), (7, 4, 2)),     # digits 3 + 3 + 1; 3 + 1; 2 of 3
}


@functools.lru_cache(maxsize=None)
def chain(cid):
    N, L, shape, _ = CHAINS[cid]
    q, psi = O.params_generate(N, L, 52, 60)
    dn, al, p, _ = O.special_primes(N, q)
    assert (dn, al, len(p)) == shape
    s, e, a = O.sample_keygen(SEED, N, q)
    sk, pk = O.keygen(s, e, a, q, psi)
    return dict(N=N, L=L, q=q, psi=psi, sk=sk, pk=pk, evk=O.evk_keygen(SEED, sk, q, psi))


@pytest.mark.parametrize("cid,Ll", [(cid, Ll) for cid, c in CHAINS.items() for Ll in c[3]], ids=str)
def test_identity_automorphism_is_the_oracles_key_switch(cid, Ll):
    x = chain(cid)
    N, q, psi = x["N"], x["q"], x["psi"]
    rng = np.random.default_rng([Ll, len(cid)])
    c = _residue_batch(rng, q, 1, Ll, N)[0, 0]
    c[:, :4] = (q[:Ll] - np.uint64(1))[:, None]
    c[:, 4:8] = 0
    X, Y = np.zeros((1, 2, Ll, N), np.uint64), np.zeros((1, 2, Ll, N), np.uint64)
    X[0, 1], Y[0, 1] = c, 1
    # any key in the evaluation key's layout: the oracle's own, and uniform residues
    T0 = x["evk"].shape[2]
    _, _, p, _ = O.special_primes(N, q)
    mods = [int(v) for v in q] + [int(v) for v in p]
    rnd = np.stack([rng.integers(0, mods[t], x["evk"].shape[:2] + (N,), dtype=np.uint64) for t in range(T0)], axis=2)
    for key in (x["evk"], rnd):
        exp = O.eval_mult(X, Y, key, q, psi)[0]
        got = H.key_switch_hoisted(H.decompose(c, q, psi), 1, key, q, psi)
        assert np.array_equal(got, exp)


@pytest.mark.parametrize("slots", [1 << 10, 1 << 7], ids=["full", "sparse"])
def test_hoisted_rotations_decrypt_to_rolled_slots(slots):
    x = chain("two_digits")
    N, q, psi, sk = x["N"], x["q"], x["psi"], x["sk"]
    delta = float(q[-1])
    x2 = np.random.default_rng(slots).uniform(-1, 1, 2 * slots)  # K = 2
    ct = O.encrypt_vector(x2, x["pk"], q, psi, N, slots, delta, SEED)
    xs = x2.reshape(2, slots)
    rs = [1, 0, -2, slots - 1, 1]
    keys = {r: R.rot_key_from_evk(x["evk"], r, sk, q, psi) for r in set(rs) if r}
    out = H.hoisted_ref(ct, rs, keys, q, psi)
    assert out.shape == (len(rs),) + ct.shape
    assert np.array_equal(out[1], ct) and np.array_equal(out[0], out[4])
    tol = max(1e-7, 2.0 ** (18 - 52))
    for i, r in enumerate(rs):
        dec = O.decrypt_vector(out[i], sk, q, psi, slots, delta, 2 * slots).reshape(2, slots)
        err = np.abs(dec - np.roll(xs, -r, axis=1)).max()
        print("hoisted r=%d: max error %.3g" % (r, err))
        assert err < tol
    # a valid rotation, but not rotate's residues
    for i, r in ((0, 1), (2, -2)):
        ref = R.rotate_ref(ct, r, keys[r], q, psi)
        assert not np.array_equal(out[i], ref)
        assert (out[i] != ref).mean() > 0.9  # the key switch's rounding differs everywhere, in both components


def test_hoisted_rotation_at_a_truncated_level():
    x = chain("three_digits")
    N, q, psi, sk = x["N"], x["q"], x["psi"], x["sk"]
    slots, delta = N // 2, float(q[-1])
    v = np.random.default_rng(5).uniform(-1, 1, slots)
    ct = O.encrypt_vector(v, x["pk"], q, psi, N, slots, delta, SEED)[:, :, :4]
    keys = {-2: R.rot_key_from_evk(x["evk"], -2, sk, q, psi)}
    out = H.hoisted_ref(ct, [-2], keys, q, psi)
    dec = O.decrypt_vector(out[0], sk[:4], q[:4], psi[:4], slots, delta, slots)
    assert np.abs(dec - np.roll(v, 2)).max() < 1e-7
