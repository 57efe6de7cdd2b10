"""SURVEY §8 f4 on the MI355X at every level, digit shape and edge: EvalMult with HYBRID
relinearization and ModReduce, bit for bit against the oracle (checked on these shapes by
tests/test_oracle_f4_levels.py), on raw [K][2][Ll][N] residues.

tests/test_gpu_f4.py multiplies fresh ciphertexts at K = 2, at the top level and one below,
on chains of at most 6 towers.  Here every level Ll = L..1 of each chain runs, so the per-level
tables of eval.cpp (extended basis, per-digit foreign towers, conversion constants) are built
and used where a digit disappears (dn < dnum: the key is indexed with the full chain's dnum
and tower count), where the last digit shrinks to one tower, and at Ll = 1:

  A  2^12, 7 towers   alpha 3, kP 3: modup_kernel + a columns pass per digit over its foreign
                      towers, moddown_kernel + columns, the compile-time inner / finish kernels
  B  2^11, 7 towers   the same digits on a single-block ring (no columns pass)
  C  2^12, 12 towers  alpha 4, kP 4, T = Ll + kP = 16 (kMaxTowers) at the top
  D  2^13, 6 towers   fused modup_cols<2> / moddown_cols<2>, partial digits (5, 3, 1 towers)
  E  2^16, 6 towers   LOGR = 5 (unfused) with dn < dnum, at levels 4 and 1
  F  2^17, 5 towers   three digits of 2^12-element blocks: the 96 KiB inner product
  G  2^12, 4 towers   30-bit towers (red_ok false): the generic kernels, where red128's high
                      word exceeds q_t
  H  2^12, 13 towers  L + kP = 18: EvalMult is refused; ModReduce and decrypt still work

Operand classes: "uniform" (residues uniform below each modulus) and "edges" (all q_t - 1;
all 0 against q_t - 1; a c2 planted with 0, 1 and Q_j - 1 in whole digits), at K = 3 wherever
the ring is small (odd K in the row / Ll, k T + t and ext_base arithmetic).  E and F stay at
exactly the listed levels and K = 1: the oracle takes seconds per product there."""
import functools

import numpy as np
import pytest

import oracle as O
from f4_cases import (DEFECT_CAP, _edge_batch, _planted_rescale_input, _relin_defect, _rescale_coeffs,
                      _residue_batch)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

# id: (ring, towers, scale bits, first modulus bits, (dnum, alpha, kP), levels, K)
CHAINS = {
    "A": (1 << 12, 7, 52, 60, (3, 3, 3), range(7, 0, -1), 3),
    "B": (1 << 11, 7, 52, 60, (3, 3, 3), range(7, 0, -1), 3),
    "C": (1 << 12, 12, 52, 60, (3, 4, 4), range(12, 0, -1), 1),
    "D": (1 << 13, 6, 52, 60, (3, 2, 2), range(6, 0, -1), 3),
    "E": (1 << 16, 6, 52, 60, (3, 2, 2), (4, 1), 1),
    "F": (1 << 17, 5, 52, 60, (3, 2, 2), (5,), 1),
    "G": (1 << 12, 4, 30, 45, (2, 2, 2), range(4, 0, -1), 3),
}
LEVELS = [(cid, Ll) for cid, c in CHAINS.items() for Ll in c[5]]
DEFECT_CHAINS = "ABCDG"  # the relinearization identity on the GPU's output (small rings)


def _ids(v):
    return str(v)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _make(N, L, sb, fb, seed):
    c = m.CKKS("ckks", N // 2, sb, "", multDepth=L - 1, firstModBits=fb, ringDim=N, seed=seed, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    assert (inf["ring_dim"], inf["num_towers"]) == (N, L)
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    pk, sk = c.get_keys()
    return dict(c=c, inf=inf, q=q, psi=psi, sk=sk, N=N, L=L, seed=seed)


@functools.lru_cache(maxsize=None)
def chain(cid):
    """One context per chain for the whole module, with its evaluation key."""
    N, L, sb, fb = CHAINS[cid][:4]
    x = _make(N, L, sb, fb, 700 + ord(cid))
    x["c"].evalMultKeyGen()
    x["evk"] = x["c"].get_eval_key()
    x["K"] = CHAINS[cid][6]
    x["alpha"] = CHAINS[cid][4][1]
    return x


def _rng(cid, Ll, salt):
    return np.random.default_rng([ord(cid), Ll, salt])


@pytest.mark.parametrize("cid", list(CHAINS))
def test_eval_key_and_digit_shape(cid):
    x = chain(cid)
    c, q, psi = x["c"], x["q"], x["psi"]
    dn, al, p, _ = O.special_primes(x["N"], q)
    assert (dn, al, len(p)) == CHAINS[cid][4]
    info = c.eval_key_info()
    assert info["has_key"] and (info["dnum"], info["alpha"]) == (dn, al)
    assert info["special_moduli"] == [int(v) for v in p]
    assert x["evk"].shape == (2, dn, x["L"] + len(p), x["N"])
    assert np.array_equal(x["evk"], O.evk_keygen(x["seed"], x["sk"], q, psi))


@pytest.mark.parametrize("cid,Ll", LEVELS, ids=_ids)
def test_mult_uniform(cid, Ll):
    x = chain(cid)
    rng = _rng(cid, Ll, 1)
    a, b = (_residue_batch(rng, x["q"], x["K"], Ll, x["N"]) for _ in range(2))
    got = _u64(D.mult(x["c"], _dev(a), _dev(b)))
    assert np.array_equal(got, O.eval_mult(a, b, x["evk"], x["q"], x["psi"]))


@pytest.mark.parametrize("cid,Ll", LEVELS, ids=_ids)
def test_mult_edges(cid, Ll):
    """All q_t - 1 (the tensor kernel's and red128's largest sums), all 0 against q_t - 1, and a
    c2 whose digits hold 0, 1 and Q_j - 1 — equal to the oracle, and on the small rings within
    the derived cap of the relinearization identity under the context's secret key."""
    x = chain(cid)
    a, b = _edge_batch(_rng(cid, Ll, 2), x["q"], x["psi"], Ll, x["alpha"], x["N"], x["K"])
    got = _u64(D.mult(x["c"], _dev(a), _dev(b)))
    assert np.array_equal(got, O.eval_mult(a, b, x["evk"], x["q"], x["psi"]))
    if cid in DEFECT_CHAINS:
        d = _relin_defect(got, a, b, x["sk"], x["q"], x["psi"])
        print("max|d| %s Ll=%d: %d" % (cid, Ll, d))
        assert d < DEFECT_CAP


@pytest.mark.parametrize("cid,Ll", [v for v in LEVELS if v[1] >= 2], ids=_ids)
def test_rescale_uniform_and_lift_boundary(cid, Ll):
    """ModReduce of uniform residues, and of coefficients planted at the centred lift's
    boundary (last-tower residues 0, 1, (q_l - 1)/2, (q_l + 1)/2, q_l - 1): equal to the
    oracle, and the planted one equal to the integer rounding division."""
    x = chain(cid)
    c, q, psi, N = x["c"], x["q"], x["psi"], x["N"]
    rng = _rng(cid, Ll, 3)
    planted, exp = _planted_rescale_input(rng, q, psi, Ll, N)
    K = max(2, x["K"])  # uniform ciphertexts, then the planted one
    ct = np.concatenate([_residue_batch(rng, q, K - 1, Ll, N), planted])
    got = _u64(D.rescale(c, _dev(ct)))
    assert got.shape == (K, 2, Ll - 1, N)
    assert np.array_equal(got, O.rescale(ct, q, psi))
    assert np.array_equal(_rescale_coeffs(got[-1], q, psi), exp)


def test_walk_down_chain_a():
    """Square and rescale real ciphertexts from 7 towers to 1: every product and every
    ModReduce bit-exact against the oracle, every level's decode within the tolerance rule of
    tests/test_gpu_f4.py (x^64 at one tower is the last decodable level: the product there,
    at scale ~2^104 over a 60-bit modulus, is still bit-exact but holds no value)."""
    x = chain("A")
    c, q, psi, sk, evk, inf = x["c"], x["q"], x["psi"], x["sk"], x["evk"], x["inf"]
    S, n = inf["batch"], 3 * inf["batch"]
    vals = np.random.default_rng(7).uniform(-1, 1, n)
    ct = D.encrypt(c, torch.tensor(vals, dtype=torch.float64, device="cuda"))
    assert ct.shape[0] == 3
    scale = inf["delta"]
    tol = max(1e-7, 2.0 ** (18 - inf["scale_bits"]))
    for Ll in range(7, 0, -1):
        sq = D.mult(c, ct, ct)
        ref = O.eval_mult(_u64(ct), _u64(ct), evk, q, psi)
        assert np.array_equal(_u64(sq), ref), Ll
        if Ll == 1:
            break
        ct = D.rescale(c, sq)
        assert np.array_equal(_u64(ct), O.rescale(ref, q, psi)), Ll
        scale = scale * scale / float(q[Ll - 1])
        vals = vals * vals
        dec = D.decrypt(c, ct, n, scale).cpu().numpy()
        assert np.array_equal(dec, O.decrypt_vector(_u64(ct), sk[:Ll - 1], q[:Ll - 1], psi[:Ll - 1], S, scale, n))
        err = float(np.abs(dec - vals).max())
        print("walk: %d towers, max error %.3g" % (Ll - 1, err))
        assert err < tol, Ll


def test_aliasing_and_square():
    """The documented exact aliasing (out is a, out is b) and a is b, on chain D at level 4
    (two digits of the full three), K = 3."""
    x = chain("D")
    c = x["c"]
    rng = _rng("D", 4, 4)
    a, b = (_residue_batch(rng, x["q"], 3, 4, x["N"]) for _ in range(2))
    ref = _u64(D.mult(c, _dev(a), _dev(b)))
    assert np.array_equal(ref, O.eval_mult(a, b, x["evk"], x["q"], x["psi"]))
    ta, tb = _dev(a), _dev(b)
    assert D.mult(c, ta, tb, out=ta) is ta
    assert np.array_equal(_u64(ta), ref) and np.array_equal(_u64(tb), b)
    ta, tb = _dev(a), _dev(b)
    D.mult(c, ta, tb, out=tb)
    assert np.array_equal(_u64(tb), ref) and np.array_equal(_u64(ta), a)
    ta = _dev(a)
    sq = O.eval_mult(a, a, x["evk"], x["q"], x["psi"])
    assert np.array_equal(_u64(D.mult(c, ta, ta)), sq)
    D.mult(c, ta, ta, out=ta)
    assert np.array_equal(_u64(ta), sq)


def test_chain_too_long_for_key_switching():
    """13 towers need 5 special primes: 18 towers exceed the 16 the kernels hold, so the
    evaluation key is refused by name — and ModReduce and decrypt, which need only the Q_l
    tables, still work at any level of that chain."""
    x = _make(1 << 12, 13, 52, 60, 913)
    c, q, psi, sk, N = x["c"], x["q"], x["psi"], x["sk"], x["N"]
    dn, al, p, _ = O.special_primes(N, q)
    assert (dn, al, len(p)) == (3, 5, 5)
    info = c.eval_key_info()
    assert (info["dnum"], info["alpha"], len(info["special_moduli"]), info["has_key"]) == (3, 5, 5, False)
    with pytest.raises((ValueError, RuntimeError), match="<= 16"):
        c.evalMultKeyGen()
    with pytest.raises((ValueError, RuntimeError), match="<= 16"):
        c.set_eval_key(np.zeros((2, dn, 13 + len(p), N), np.uint64))
    rng = np.random.default_rng(13)
    top = _residue_batch(rng, q, 1, 13, N)
    with pytest.raises((ValueError, RuntimeError)):  # no key can exist
        D.mult(c, _dev(top), _dev(top))
    assert not c.eval_key_info()["has_key"]
    for Ll in (13, 2):
        planted, exp = _planted_rescale_input(rng, q, psi, Ll, N)
        ct = np.concatenate([_residue_batch(rng, q, 2, Ll, N), planted])
        got = _u64(D.rescale(c, _dev(ct)))
        assert np.array_equal(got, O.rescale(ct, q, psi))
        assert np.array_equal(_rescale_coeffs(got[-1], q, psi), exp)
    S, n, d = x["inf"]["batch"], 3 * x["inf"]["batch"], x["inf"]["delta"]
    vals = rng.uniform(-1, 1, n)
    ct = D.encrypt(c, torch.tensor(vals, dtype=torch.float64, device="cuda"))[:, :, :3].contiguous()
    dec = D.decrypt(c, ct, n, d).cpu().numpy()
    assert np.array_equal(dec, O.decrypt_vector(_u64(ct), sk[:3], q[:3], psi[:3], S, d, n))
    assert np.abs(dec - vals).max() < 1e-7
