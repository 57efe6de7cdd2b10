"""The plaintext-operand calls without a device: tests/plain_ref.py, the yardstick
tests/test_gpu_plain_ops.py compares the kernels with bit for bit, checked here for what it must mean,
against the oracle alone -- the oracle's decrypt of an oracle ciphertext combined with an oracle
plaintext gives the slot-wise product, sum and difference.

Scale bookkeeping (the API carries none): a factor encoded over the ciphertext's l towers at scale
float(q[l - 1]) makes a product of scale delta * q[l - 1]; ModReduce divides by q[l - 1], so the result
is back at delta over l - 1 towers.  An addend is encoded at the ciphertext's own scale.

Tolerances: both contexts have 52-bit scaling primes.  A product after ModReduce is judged by the rule
tests/test_gpu_f4.py uses for EvalMult, max(1e-7, 2^(18 - scaleBits)) = 1e-7; a sum or difference adds
an exact encoding (rounding error 2^-53 per coefficient) to a fresh ciphertext, whose own error
(sigma 3.19 noise over 2^52, times the decode's sqrt(N) spread) is below 2^-40: 1e-7 as for the
fresh ciphertexts of tests/test_rotation_ref.py."""
import functools

import numpy as np
import pytest

import oracle as O
import plain_ref as P

SEED = 131
# (N, L, towers the ciphertext has when the plaintext meets it)
CASES = {"2^11/L2": (1 << 11, 2, 2), "2^13/L3@2": (1 << 13, 3, 2)}
TOL_MULT = max(1e-7, 2.0 ** (18 - 52))
TOL_ADD = 1e-7


@functools.lru_cache(maxsize=None)
def _case(name):
    """Oracle keys, K = 2 fresh ciphertexts of x cut to l towers (dropping towers of a ciphertext is
    exact: c0 + c1 s = m + e holds modulo every divisor of Q, at the same scale), and y."""
    N, L, l = CASES[name]
    S = N // 2
    q, psi = O.params_generate(N, L, 52, 60)
    s, e, a = O.sample_keygen(SEED, N, q)
    sk, pk = O.keygen(s, e, a, q, psi)
    delta = float(int(q[-1]))
    rng = np.random.default_rng(l * N)
    x, y = rng.uniform(-1, 1, 2 * S), rng.uniform(-1, 1, 2 * S)
    ct = O.encrypt_vector(x, pk, q, psi, N, S, delta, SEED)[:, :, :l].copy()
    return dict(N=N, S=S, l=l, q=q, psi=psi, sk=sk, delta=delta, x=x, y=y, ct=ct)


def _encode(c, y, scale):
    l = c["l"]
    return np.stack([O.encode(y[k * c["S"]:(k + 1) * c["S"]], c["N"], c["S"], scale, c["q"][:l], c["psi"][:l])
                     for k in range(len(y) // c["S"])])


def _decrypt(c, ct, scale):
    l = ct.shape[2]
    return O.decrypt_vector(ct, c["sk"][:l], c["q"][:l], c["psi"][:l], c["S"], scale, ct.shape[0] * c["S"])


@pytest.mark.parametrize("name", list(CASES))
def test_truncated_ciphertext_decrypts_to_x(name):
    c = _case(name)
    assert np.abs(_decrypt(c, c["ct"], c["delta"]) - c["x"]).max() < TOL_ADD


@pytest.mark.parametrize("name", list(CASES))
def test_mult_plain_then_rescale_decrypts_to_the_product(name):
    c = _case(name)
    l, q = c["l"], c["q"]
    pt = _encode(c, c["y"], float(int(q[l - 1])))
    prod = P.mult_plain(c["ct"], pt, q)
    assert prod.shape == c["ct"].shape and all((prod[:, :, t] < q[t]).all() for t in range(l))
    res = O.rescale(prod, q, c["psi"])
    assert res.shape[2] == l - 1
    assert np.abs(_decrypt(c, res, c["delta"]) - c["x"] * c["y"]).max() < TOL_MULT
    # one plaintext for every ciphertext (Kp = 1, and the [l][N] form)
    for one in (pt[:1], pt[0]):
        prod1 = P.mult_plain(c["ct"], one, q)
        assert np.array_equal(prod1[0], prod[0])
        y1 = np.tile(c["y"][:c["S"]], 2)
        assert np.abs(_decrypt(c, O.rescale(prod1, q, c["psi"]), c["delta"]) - c["x"] * y1).max() < TOL_MULT


@pytest.mark.parametrize("name", list(CASES))
def test_add_and_sub_plain_decrypt_to_sum_and_difference(name):
    c = _case(name)
    q = c["q"]
    pt = _encode(c, c["y"], c["delta"])
    for fn, exp in ((P.add_plain, c["x"] + c["y"]), (P.sub_plain, c["x"] - c["y"])):
        out = fn(c["ct"], pt, q)
        assert np.array_equal(out[:, 1], c["ct"][:, 1])  # c1 passes through
        assert np.abs(_decrypt(c, out, c["delta"]) - exp).max() < TOL_ADD
    y1 = np.tile(c["y"][:c["S"]], 2)
    assert np.abs(_decrypt(c, P.add_plain(c["ct"], pt[0], q), c["delta"]) - (c["x"] + y1)).max() < TOL_ADD


@pytest.mark.parametrize("name", list(CASES))
def test_sub_and_neg(name):
    c = _case(name)
    q, ct = c["q"], c["ct"]
    a, b = ct[:1], ct[1:]
    S = c["S"]
    assert np.abs(_decrypt(c, P.sub(a, b, q), c["delta"]) - (c["x"][:S] - c["x"][S:])).max() < TOL_ADD
    assert np.abs(_decrypt(c, P.neg(ct, q), c["delta"]) + c["x"]).max() < TOL_ADD
    assert not P.sub(ct, ct, q).any()
    assert np.array_equal(P.neg(P.neg(ct, q), q), ct)


def test_canonical_outputs_at_the_planted_edges():
    """0, 1, q - 1, q - 2 against 0 and q - 1: every result is below q_t, the negation of 0 is 0, and
    (q - 1)(q - 1) = 1."""
    c = _case("2^11/L2")
    q, l = c["q"], c["l"]
    ct = P.plant(c["ct"].copy(), q, P.CT_EDGES, div=4)
    pt = P.plant(_encode(c, c["y"], c["delta"]), q, P.PT_EDGES)
    for out in (P.mult_plain(ct, pt, q), P.add_plain(ct, pt, q), P.sub_plain(ct, pt, q), P.sub(ct, ct[::-1], q),
                P.neg(ct, q)):
        assert all((out[:, :, t] < q[t]).all() for t in range(l))
    assert (P.mult_plain(ct, pt, q)[:, :, :, 0] == 1).all()  # (q - 1)(q - 1)
    assert (P.mult_plain(ct, pt, q)[:, :, :, 4] == 0).all()  # 0 (q - 1)
    assert (P.neg(ct, q)[:, :, :, 4] == 0).all() and (P.neg(ct, q)[:, :, :, 0] == 1).all()
    assert (P.add_plain(ct, pt, q)[:, 0, :, 2] == 0).all()   # (q - 1) + 1
    assert all((P.sub_plain(ct, pt, q)[:, 0, t, 6] == int(q[t]) - 1).all() for t in range(l))  # 0 - 1
