"""SURVEY §8 f4 on the CPU, at every level: the oracle's EvalMult / ModReduce checked where
tests/test_gpu_f4_levels.py leans on it — digits of 3 and 4 towers, 3 and 4 special primes,
T = Ll + kP = 16, levels that lose a digit, a last digit of one tower, Ll = 1, and 30-bit
towers under 60-bit special primes.  tests/test_oracle_f4.py checks one L = 3, alpha = 2
chain at two levels; on the shapes here the oracle would otherwise be an unchecked reference.

Nothing here needs key files: the keys come from the oracle's own seeded samplers.  The
checks are exact integer statements (the relinearization identity with a derived cap,
ModReduce as a rounding division), plus decryption to the plaintext products."""
import functools

import numpy as np
import pytest

import oracle as O
from f4_cases import (DEFECT_CAP, _planted_rescale_input, _relin_defect, _rescale_coeffs,
                      _residue_batch)

# id: (ring, towers, scale bits, first modulus bits, (dnum, alpha, kP))
CHAINS = {
    "n11_L7": (1 << 11, 7, 52, 60, (3, 3, 3)),
    "n12_L12": (1 << 12, 12, 52, 60, (3, 4, 4)),  # T = 16 at the top level
    "n12_L6": (1 << 12, 6, 52, 60, (3, 2, 2)),
    "n11_L4_30bit": (1 << 11, 4, 30, 45, (2, 2, 2)),  # 30-bit towers under 60-bit special primes
}
LEVELS = [(cid, Ll) for cid, c in CHAINS.items() for Ll in range(c[1], 0, -1)]


@functools.lru_cache(maxsize=None)
def chain(cid):
    N, L, sb, fb, _ = CHAINS[cid]
    q, psi = O.params_generate(N, L, sb, fb)
    s, e, a = O.sample_keygen(11 + L, N, q)
    sk, pk = O.keygen(s, e, a, q, psi)
    evk = O.evk_keygen(11 + L, sk, q, psi)
    return dict(N=N, L=L, sb=sb, q=q, psi=psi, sk=sk, pk=pk, evk=evk)


@pytest.mark.parametrize("cid", list(CHAINS))
def test_digit_shapes(cid):
    N, L, sb, fb, shape = CHAINS[cid]
    c = chain(cid)
    dn, al, p, pr = O.special_primes(N, c["q"])
    assert (dn, al, len(p)) == shape
    assert all(int(v).bit_length() == 60 for v in p) and not set(map(int, p)) & set(map(int, c["q"]))
    assert c["evk"].shape == (2, dn, L + len(p), N)


@pytest.mark.parametrize("cid,Ll", LEVELS, ids=lambda v: str(v))
def test_relinearization_identity(cid, Ll):
    """out0 + out1 s = c0 + c1 s + c2 s^2 + d with |d| < 2^24 (f4_cases.DEFECT_CAP: derived from
    the key's error bound, below 2^22 here), for uniform operands at every level.  A wrong
    residue anywhere makes d uniform modulo Q_l >= 2^45.
    Measured max |d| over the levels (7 to 8 bits, the same at every level): n11_L7 141,
    n12_L12 199, n12_L6 122, n11_L4_30bit 110."""
    c = chain(cid)
    rng = np.random.default_rng(100 * Ll + c["L"])
    A, B = (_residue_batch(rng, c["q"], 1, Ll, c["N"]) for _ in range(2))
    out = O.eval_mult(A, B, c["evk"], c["q"], c["psi"])
    assert all(int(out[:, :, t].max()) < int(c["q"][t]) for t in range(Ll))
    d = _relin_defect(out, A, B, c["sk"], c["q"], c["psi"])
    print("max|d| %s Ll=%d: %d" % (cid, Ll, d))
    assert d < DEFECT_CAP


@pytest.mark.parametrize("cid,Ll", [(cid, Ll) for cid, Ll in LEVELS if Ll >= 3], ids=lambda v: str(v))
def test_products_decrypt_at_every_level(cid, Ll):
    """Two fresh ciphertexts sliced to Ll towers, multiplied: the product decodes at scale
    delta^2 to x y within 1e-9 (52-bit scale; measured at most 5.1e-12 at 2^11, 1.7e-11 at
    2^12) or 1e-3 (30-bit scale, levels 3 and 4; measured 2.6e-5)."""
    c = chain(cid)
    N, S, q, psi = c["N"], c["N"] // 2, c["q"], c["psi"]
    delta = 2.0 ** c["sb"]
    rng = np.random.default_rng(Ll)
    x, y = (rng.uniform(-1, 1, S) for _ in range(2))
    cx = O.encrypt_vector(x, c["pk"], q, psi, N, S, delta, seed=5, g0=0)[:, :, :Ll].copy()
    cy = O.encrypt_vector(y, c["pk"], q, psi, N, S, delta, seed=5, g0=1)[:, :, :Ll].copy()
    m = O.eval_mult(cx, cy, c["evk"], q, psi)
    dec = O.decrypt_vector(m, c["sk"][:Ll], q[:Ll], psi[:Ll], S, delta * delta, S)
    err = float(np.abs(dec - x * y).max())
    print("decode error %s Ll=%d: %.3g" % (cid, Ll, err))
    assert err < (1e-9 if c["sb"] == 52 else 1e-3)


@pytest.mark.parametrize("Ll", range(7, 1, -1))
def test_rescale_rounds_at_the_lift_boundary(Ll):
    """ModReduce at every level of the L = 7 chain on coefficients c = k q_l + r with r at 0, 1,
    (q_l - 1)/2, (q_l + 1)/2 and q_l - 1 (k zero, negative and positive): every remaining tower
    is floor((2c + q_l) / (2 q_l)) mod q_t.  A lift that took (q_l - 1)/2 as negative would be
    off by one there."""
    c = chain("n11_L7")
    ct, exp = _planted_rescale_input(np.random.default_rng(Ll), c["q"], c["psi"], Ll, c["N"])
    out = O.rescale(ct, c["q"], c["psi"])
    assert out.shape == (1, 2, Ll - 1, c["N"])
    assert np.array_equal(_rescale_coeffs(out[0], c["q"], c["psi"]), exp)
