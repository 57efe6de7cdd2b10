"""tests/seeded_ref.py checked for meaning on the CPU: its 128-bit draw is keygen's, pinned
to the oracle's C on three modulus classes, and the ciphertext it restates decrypts under the oracle."""
import numpy as np
import pytest

import oracle as O
import seeded_ref as R


def _prime(bits, N):
    """The largest prime below 2^bits that is 1 mod 2N (a tower modulus of that class)."""
    q = (1 << bits) - (1 << bits) % (2 * N) + 1
    while q >= 1 << bits or not _is_prime(q):
        q -= 2 * N
    return q


def _is_prime(n):
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):  # deterministic below 3.3e24
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def test_the_draw_matches_keygen():
    N, s = 1024, 31
    q = [_prime(b, N) for b in (30, 52, 60)]
    assert [int(v).bit_length() for v in q] == [30, 52, 60]
    a = O.sample_keygen(s, N, q)[2]
    key = O.seed_to_key(s)
    for t, qt in enumerate(q):
        assert np.array_equal(R.uniform_draw(key, (2 << 56) | (1 + t), N, qt), a[t]), qt


def test_nonce_and_seed_layout():
    assert R.nonce(0, 0) == 9 << 56 and R.nonce(5, 3) == (9 << 56) | (5 << 8) | 3
    with pytest.raises(AssertionError):
        R.nonce(1 << 48, 0)
    seed = R.call_seed(7, 3)
    assert len(seed) == 32 and seed != R.call_seed(7, 4) and seed != R.call_seed(8, 3)
    # the seed is a block of the stream key, never the key itself
    assert seed != O.seed_to_key(7).astype("<u4").tobytes()
    assert np.array_equal(R.seed_words(seed), O.chacha20_block(O.seed_to_key(7), 0, (9 << 56) | 3)[:8])
    # one ciphertext's towers and one tower's ciphertexts draw from different blocks
    q = [_prime(52, 1024)] * 2
    e0, e1 = R.expand(seed, 0, q, 1024), R.expand(seed, 1, q, 1024)
    assert not np.array_equal(e0[0], e0[1]) and not np.array_equal(e0[0], e1[0])
    assert (e0 < np.uint64(q[0])).all()
    assert R.expand_blocks(seed, 1, 1, q[1], [0, 255]) == {0: [int(v) for v in e1[1][:4]],
                                                           255: [int(v) for v in e1[1][1020:]]}


@pytest.mark.parametrize("N,slots", [(2048, 1024), (2048, 256)], ids=["full", "gap4"])
def test_the_restated_ciphertext_decrypts(N, slots):
    L, seed_int, g, k = 2, 11, 4, 2
    q, psi = O.params_generate(N, L)
    delta = float(int(q[-1]))
    s, e, a = O.sample_keygen(seed_int, N, q)
    sk, _ = O.keygen(s, e, a, q, psi)
    x = np.random.default_rng(1).uniform(-1, 1, slots)
    seed = R.call_seed(seed_int, g - k)
    ct = R.encrypt_seeded(x, sk, seed_int, g, seed, k, N, slots, delta, q, psi)
    assert ct.shape == (2, L, N) and np.array_equal(ct[1], R.expand(seed, k, q, N))
    got = O.decrypt(ct, sk, q, psi, slots, delta, slots)
    # a slot's error is a sum of N coefficient errors, each at most T + 1/2 (|e| <= T, the rounding), over Delta
    T = len(O.gauss_cdt())
    bound = N * (T + 1) / delta + 1e-12
    assert np.abs(got - x).max() <= bound
    # under another ciphertext's stream the same c0 is not a ciphertext of x
    bad = np.stack([ct[0], R.expand(seed, k + 1, q, N)])
    assert np.abs(O.decrypt(bad, sk, q, psi, slots, delta, slots) - x).max() > 1.0


def test_blob_payload_is_the_first_group_of_the_packed_format():
    import arena_layout as A

    N = 1024
    q = [_prime(60, N), _prime(52, N)]
    rng = np.random.default_rng(2)
    c0s = [np.stack([rng.integers(0, qt, N, dtype=np.uint64) for qt in q]) for _ in range(3)]
    pay = R.blob_payload(c0s, q, N)
    assert len(pay) == 3 * R.packed_poly_bytes(q, N) == 3 * N * sum(A.widths(q)) // 8
    for k, c0 in enumerate(c0s):
        grp = np.frombuffer(pay, np.uint32)[k * len(pay) // 12:(k + 1) * len(pay) // 12]
        back = A.unpack_arena(np.concatenate([grp, grp]), 1, 1, len(q), N, q)[0]
        assert np.array_equal(back[0, 0], c0) and np.array_equal(back[0, 1], c0)
