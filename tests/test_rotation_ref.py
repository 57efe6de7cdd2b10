"""Slot rotations and EvalSum without a device: the library's Galois elements, and
the yardstick tests/test_gpu_rotate.py measures the kernels with (tests/rotation_ref.py) checked for
what it must mean -- a reference rotation decrypts to the rolled slots and a reference EvalSum to the
sliding sums, at full and at sparse packing.

Also the two yardsticks of tests/test_gpu_rotate_gather.py: with c1 = 0 a reference rotation is the pure
gather of c0 beside a zero component under any key, and the device's 32-bit form of the gather index
(dev_common.h galois_src, restated here in numpy) is R.gather_index on every ring for the swept indices."""
import functools

import numpy as np
import pytest

import oracle as O
import rotation_ref as R

N, L, SEED = 1 << 11, 2, 77


def test_galois_element_matches_the_definition():
    import SHELFI_FHE as m

    for logn in range(11, 18):
        n = 1 << logn
        batch = n // 2
        for r in (1, -1, 2, -2, batch - 1):
            g = m.galois_element(n, r)
            assert g == R.galois(n, r), (n, r)
            assert g % 2 == 1 and g * m.galois_element(n, -r) % (2 * n) == 1
        assert m.galois_element(n, 0) == 1
        for r in (batch, -batch, batch + 5):
            with pytest.raises(ValueError):
                m.galois_element(n, r)
    with pytest.raises(ValueError):
        m.galois_element(3000, 1)


@functools.lru_cache(maxsize=None)
def _keys():
    q, psi = O.params_generate(N, L, 52, 60)
    s, e, a = O.sample_keygen(SEED, N, q)
    sk, pk = O.keygen(s, e, a, q, psi)
    evk = O.evk_keygen(SEED, sk, q, psi)
    return q, psi, sk, pk, evk


def test_gather_form_of_the_automorphism():
    """The kernels' index map against the coefficient-domain definition, r > 0 and r < 0, and its
    locality: aligned runs of 2^k positions map onto aligned runs."""
    q, psi = _keys()[:2]
    x = np.random.default_rng(1).integers(0, int(q[0]), N, dtype=np.uint64)
    for r in (1, -1, -2, 5, N // 2 - 1):
        g = R.galois(N, r)
        src = R.gather_index(N, g)
        assert np.array_equal(np.sort(src), np.arange(N))
        assert np.array_equal(x[src], R.sigma_eval(x[None], g, q, psi)[0])
        for k in (1, 5, 8):
            assert np.array_equal(src >> k, (src >> k)[::1 << k].repeat(1 << k))


@pytest.mark.parametrize("slots", [N // 2, N // 8], ids=["full", "sparse"])
def test_reference_rotation_and_eval_sum_decrypt_to_rolled_slots(slots):
    q, psi, sk, pk, evk = _keys()
    delta = float(q[-1])
    rng = np.random.default_rng(slots)
    x = rng.uniform(-1, 1, 2 * slots)  # K = 2
    ct = O.encrypt_vector(x, pk, q, psi, N, slots, delta, SEED)
    assert ct.shape == (2, 2, L, N)
    xs = x.reshape(2, slots)
    for r in (1, -2, slots - 1):
        key = R.rot_key_from_evk(evk, r, sk, q, psi)
        e = R.key_error(key, r, sk, q, psi)
        assert np.abs(e).max() < 64 and e.any() and (e == e[:, :1]).all()
        rot = R.rotate_ref(ct, r, key, q, psi)
        dec = O.decrypt_vector(rot, sk, q, psi, slots, delta, 2 * slots).reshape(2, slots)
        assert np.abs(dec - np.roll(xs, -r, axis=1)).max() < 1e-7
    keys = {1 << i: R.rot_key_from_evk(evk, 1 << i, sk, q, psi) for i in range(slots.bit_length() - 1)}
    for n in (1, 4, slots):
        tot = R.eval_sum_ref(ct, n, keys, q, psi)
        dec = O.decrypt_vector(tot, sk, q, psi, slots, delta, 2 * slots).reshape(2, slots)
        exp = sum(np.roll(xs, -j, axis=1) for j in range(n))
        assert np.abs(dec - exp).max() < 1e-7 * n


def test_rotation_of_a_zero_second_component_is_the_gather_under_any_key():
    """KeySwitch(sigma_g(0)) = 0 whatever the key holds: Rotate((c0, 0), r) = (c0[..., src_g], 0), under the
    oracle's evaluation key (not a rotation key at all) and under a key made for r."""
    n, towers = 1 << 11, 3
    q, psi = O.params_generate(n, towers, 52, 60)
    s, e, a = O.sample_keygen(SEED, n, q)
    sk, _ = O.keygen(s, e, a, q, psi)
    evk = O.evk_keygen(SEED, sk, q, psi)
    rng = np.random.default_rng(3)
    ct = np.zeros((2, 2, towers, n), np.uint64)
    for t in range(towers):
        ct[:, 0, t] = rng.integers(0, int(q[t]), (2, n), dtype=np.uint64)
    batch = n // 2
    for r in (1, -3, batch // 2 + 1, batch - 1):
        src = R.gather_index(n, R.galois(n, r))
        for key in (evk, R.rot_key_from_evk(evk, r, sk, q, psi)):
            out = R.rotate_ref(ct, r, key, q, psi)
            assert not out[:, 1].any(), r
            assert np.array_equal(out[:, 0], ct[:, 0][..., src]), r


def _brev32(v):
    v = np.asarray(v, np.uint64)
    r = np.zeros_like(v)
    for i in range(32):
        r |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(31 - i)
    return r


def device_galois_src(n, g):
    """dev_common.h galois_src for every j < n, step for step: a 32-bit bit reversal shifted right by
    32 - logN, the product g e kept to its low 32 bits and then masked with 2N - 1, and the reversal again."""
    logn = n.bit_length() - 1
    m32 = np.uint64(0xFFFFFFFF)
    j = np.arange(n, dtype=np.uint64)
    e = (np.uint64(2) * (_brev32(j) >> np.uint64(32 - logn)) + np.uint64(1)) & m32
    ge = ((np.uint64(g) * e) & m32) & np.uint64(2 * n - 1)  # g, e < 2^18: the uint64 product is exact
    return (_brev32(ge >> np.uint64(1)) >> np.uint64(32 - logn)).astype(np.int64)


@pytest.mark.parametrize("logn", range(11, 18))
def test_device_form_of_the_gather_index(logn):
    n = 1 << logn
    gs = [R.galois(n, r) for r in R.sweep_indices(n // 2)]
    if logn == 15:
        gs += [R.galois(n, r) for r in R.sweep_indices(4096)]  # the sparse context's list
    assert any(g > n for g in gs) and (logn < 16 or any(g >= 1 << 16 for g in gs))
    for g in gs:
        assert np.array_equal(device_galois_src(n, g), R.gather_index(n, g)), (n, g)
