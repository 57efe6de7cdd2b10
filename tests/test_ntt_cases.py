"""tests/ntt_cases.py on the CPU: the oracle's transforms against the definition in Python integers,
    NTT(a)[i] = sum_j a_j psi^((2 bitrev(i) + 1) j) mod q,    INTT undoing it:
    a_j = N^-1 sum_i A_i psi^(-(2 bitrev(i) + 1) j) mod q,
at sampled output indices (0, N - 1, both sides of N / 2 and seeded ones) of every class, on every
modulus class and every ring up to 2^13; the sparse class returns its target exactly; every builder
lands where it claims (positions, values, canonical residues); the chains chosen for their bit
lengths have them."""
import numpy as np
import pytest

import ntt_cases as NC
import oracle as O

SMALL = [n for n in NC.SHAPES if NC.SHAPES[n][1] <= 8192]


def _bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


def _horner(coeffs, w, q):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * w + c) % q
    return acc


def _fwd_at(a, i, q, psi, logN):
    """sum_j a_j w^j, w = psi^(2 bitrev(i) + 1)."""
    return _horner(a, pow(psi, 2 * _bitrev(i, logN) + 1, q), q)


def _inv_at(A_natural, j, q, psi, N):
    """N^-1 u sum_k A[bitrev(k)] (u^2)^k, u = psi^-j; A_natural[k] = A[bitrev(k)]."""
    u = pow(pow(psi, q - 2, q), j, q)
    return pow(N, q - 2, q) * u % q * _horner(A_natural, u * u % q, q) % q


def _indices(N, seed):
    fixed = [0, N - 1, N // 2 - 1, N // 2]
    return fixed + [int(v) for v in np.random.default_rng(seed).integers(1, N - 1, 2)]


def test_shapes_cover_the_rings_and_modulus_classes():
    assert sorted({s[1] for s in NC.SHAPES.values()}) == [1 << k for k in range(10, 18)]
    for name, bits in NC.BITS.items():
        ch = NC.chain(name)
        assert [int(v).bit_length() for v in ch.q] == bits, name
    for name in NC.SHAPES:
        ch = NC.chain(name)
        for t in range(ch.L):
            q, psi = int(ch.q[t]), int(ch.psi[t])
            assert q % (2 * ch.N) == 1 and pow(psi, ch.N, q) == q - 1, (name, t)  # a primitive 2N-th root


def test_block_log(monkeypatch):
    monkeypatch.delenv("SHELFI_NTT_BLOCK_LOG_BIG", raising=False)
    assert [NC.block_log(1 << k) for k in range(10, 18)] == [10, 11, 11, 11, 11, 11, 11, 12]
    monkeypatch.setenv("SHELFI_NTT_BLOCK_LOG_BIG", "12")
    assert [NC.block_log(1 << k) for k in (15, 16, 17)] == [11, 12, 12]
    monkeypatch.setenv("SHELFI_NTT_BLOCK_LOG_BIG", "11")
    assert [NC.block_log(1 << k) for k in (15, 16, 17)] == [11, 11, 11]
    monkeypatch.setenv("SHELFI_NTT_BLOCK_LOG_BIG", "10")  # ignored, as by the library
    assert [NC.block_log(1 << k) for k in (16, 17)] == [11, 12]


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("name", SMALL)
def test_oracle_matches_the_definition(name, inverse):
    ch = NC.chain(name)
    logN = ch.N.bit_length() - 1
    br = [_bitrev(k, logN) for k in range(ch.N)]
    x, want, rows = NC.batch(name, inverse)
    for p, (cls, t) in enumerate(rows):
        q, psi = int(ch.q[t]), int(ch.psi[t])
        a = [int(v) for v in x[p]]
        if inverse:
            a = [a[k] for k in br]
        for i in _indices(ch.N, p):
            ref = _inv_at(a, i, q, psi, ch.N) if inverse else _fwd_at(a, i, q, psi, logN)
            assert int(want[p, i]) == ref, (cls, t, i)


@pytest.mark.parametrize("name", list(NC.SHAPES))
def test_builders_land_where_they_claim(name):
    ch = NC.chain(name)
    N, half = ch.N, ch.N // 2
    B = 1 << NC.block_log(N)
    for inverse in (False, True):
        x, want, rows = NC.batch(name, inverse)
        assert x.shape == want.shape == (len(NC.CLASSES) * ch.L, N)
        assert not x.flags.writeable and not want.flags.writeable
        for p, (cls, t) in enumerate(rows):
            assert t == p % ch.L and cls == NC.CLASSES[p // ch.L]
            q, psi = int(ch.q[t]), int(ch.psi[t])
            top = q - 1
            a, w = x[p], want[p]
            assert int(a.max()) < q and int(w.max()) < q, (cls, t)  # canonical in, canonical out
            do = O.ntt_inv if inverse else O.ntt_fwd
            assert np.array_equal(do(a, q, psi), w), (cls, t)
            if cls == "uniform":
                assert len(np.unique(a)) > N // 2
            elif cls == "zero":
                assert not a.any() and not w.any()
            elif cls == "full":
                assert (a == top).all()
            elif cls == "halves_lo":
                assert (a[:half] == top).all() and not a[half:].any()
            elif cls == "halves_hi":
                assert not a[:half].any() and (a[half:] == top).all()
            elif cls == "parity_ev":
                assert (a[0::2] == top).all() and not a[1::2].any()
            elif cls == "parity_od":
                assert not a[0::2].any() and (a[1::2] == top).all()
            else:
                s, pos, vals = NC.sparse_target(q, N, NC._seed(name, t, inverse) + 1)
                assert np.array_equal(w, s), "the oracle returns the sparse target exactly"
                assert len(pos) == 8 and list(np.flatnonzero(s)) == pos
                assert {0, N - 1} <= set(pos) and (B == N or {B - 1, B} <= set(pos))
                assert sorted(int(v) for v in s[pos]) == vals
                assert {1, top, top // 2, (q + 1) // 2} <= set(vals)
                assert np.count_nonzero(a) > N - 8, "a dense input"
