"""Slot rotations and EvalSum at the edges of their operands, on the chains rotation had not met
(DESIGN.md §2.11): tests/test_gpu_f4_levels.py's "edges" operand class (tests/f4_cases.py) and its chains,
bit for bit against tests/rotation_ref.py under the keys read back from the device.

  A    2^12, 7 towers   alpha 3, kP 3, every level 7 .. 1, K = 3
  C    2^12, 12 towers  alpha 4, kP 4, T = 16 at the top; levels 12, 9, 8, 5, 4, 1, K = 1
  N14  2^14, 3 towers   logN - blkLog = 3 (three column stages), every level, K = 3
  G    2^12, 4 towers   30-bit scale, 45-bit first modulus (the generic kernels), every level, K = 3
  H    2^12, 13 towers  L + kP = 18: every keyed call is refused by name, the keyless ones are exact

Operands, K = 3: all q_t - 1 in both components; c0 = 0 beside c1 all q_t - 1; a uniform c0 beside the
c1 whose image under sigma_g -- which is what the key switch sees -- is f4_cases' planted polynomial (whole
digits at 0, 1 and Q_j - 1): c1 is that polynomial under sigma of the inverse Galois element.  K = 1: the
planted one alone.  Each chain runs r = 1 and r = -2.  EvalSum (n = 4) takes the same batch on chain A at
levels 7 and 2: the accumulator's add meets q_t - 1 plus whatever the rotation returns.

On A and C the rotation keys' structure is checked as tests/test_gpu_rotate.py does: evk_combine_kernel's
Galois branch at kP = 3 and 4 and at 16 towers."""
import functools

import numpy as np
import pytest

import oracle as O
import rotation_ref as R
from f4_cases import _full_batch, _planted_c2, _residue_batch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

# id: (ring, towers, scale bits, first modulus bits, (dnum, alpha, kP), levels, K)
CHAINS = {
    "A": (1 << 12, 7, 52, 60, (3, 3, 3), range(7, 0, -1), 3),
    "C": (1 << 12, 12, 52, 60, (3, 4, 4), (12, 9, 8, 5, 4, 1), 1),
    "N14": (1 << 14, 3, 52, 60, (2, 2, 2), range(3, 0, -1), 3),
    "G": (1 << 12, 4, 30, 45, (2, 2, 2), range(4, 0, -1), 3),
}
ROTS = (1, -2)
LEVELS = [(cid, Ll, r) for cid, c in CHAINS.items() for Ll in c[5] for r in ROTS]


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
    """One context per chain for the whole module, with the keys of r = 1, -2 (and 2, for EvalSum)."""
    N, L, sb, fb = CHAINS[cid][:4]
    x = _make(N, L, sb, fb, 1200 + list(CHAINS).index(cid))
    dn, al, p, _ = O.special_primes(N, x["q"])
    assert (dn, al, len(p)) == CHAINS[cid][4]
    x["c"].rotationKeyGen([1, -2, 2])
    x["keys"] = {r: x["c"].get_rotation_key(r) for r in (1, -2, 2)}
    x["K"], x["alpha"] = CHAINS[cid][6], al
    return x


def _edge_ct(x, cid, Ll, r):
    """The edge batch [K][2][Ll][N] whose third ciphertext reaches the key switch of index r as the
    planted polynomial."""
    q, psi, N = x["q"], x["psi"], x["N"]
    rng = np.random.default_rng([len(cid), ord(cid[0]), Ll, r % 7])
    pa, _, _ = _planted_c2(rng, q, psi, Ll, x["alpha"], N)
    planted = pa.copy()
    planted[1] = R.sigma_eval(pa[1], R.galois(N, -r), q, psi)  # sigma_g of this is pa[1]
    assert np.array_equal(R.sigma_eval(planted[1, :1], R.galois(N, r), q, psi), pa[1, :1])
    if x["K"] == 1:
        return planted[None]
    return np.concatenate([_full_batch(q, 1, Ll, N), _full_batch(q, 1, Ll, N, poly0=0), planted[None]])


@pytest.mark.parametrize("cid", ["A", "C"])
def test_rotation_key_structure_on_long_chains(cid):
    """b + a s - [t in digit j] P sigma_g(s) is one small nonzero polynomial below 64 in every tower of
    Q u P, and no a row is the EvalMult key's."""
    x = chain(cid)
    c = x["c"]
    c.evalMultKeyGen()
    evk = c.get_eval_key()
    for r in ROTS:
        key = x["keys"][r]
        assert key.shape == evk.shape == (2,) + (CHAINS[cid][4][0], x["L"] + CHAINS[cid][4][2], x["N"])
        e = R.key_error(key, r, x["sk"], x["q"], x["psi"])
        assert (e == e[:, :1]).all(), r
        assert np.abs(e).max() < 64 and all(e[j].any() for j in range(e.shape[0])), r
        assert not (key[1] == evk[1]).all(axis=-1).any(), r
    assert not (x["keys"][1][1] == x["keys"][-2][1]).all(axis=-1).any()


@pytest.mark.parametrize("cid,Ll,r", LEVELS, ids=str)
def test_rotate_edges(cid, Ll, r):
    x = chain(cid)
    ct = _edge_ct(x, cid, Ll, r)
    got = _u64(D.rotate(x["c"], _dev(ct), r))
    assert np.array_equal(got, R.rotate_ref(ct, r, x["keys"][r], x["q"], x["psi"]))


@pytest.mark.parametrize("Ll", [7, 2])
def test_eval_sum_edges_chain_a(Ll):
    x = chain("A")
    ct = _edge_ct(x, "A", Ll, 1)
    got = _u64(D.eval_sum(x["c"], _dev(ct), 4))
    assert np.array_equal(got, R.eval_sum_ref(ct, 4, x["keys"], x["q"], x["psi"]))


def test_chain_too_long_for_key_switching():
    """13 towers need 5 special primes: 18 towers exceed the 16 the kernels hold.  Every call that needs
    a rotation key is refused by name and leaves no key behind; the identity rotation, EvalSum over one
    slot, EvalAdd and decrypt need none and stay exact."""
    x = _make(1 << 12, 13, 52, 60, 1213)
    c, q, psi, sk, N = x["c"], x["q"], x["psi"], x["sk"], x["N"]
    dn, al, p, _ = O.special_primes(N, q)
    assert (dn, al, len(p)) == (3, 5, 5)
    S, n, d = x["inf"]["batch"], 3 * x["inf"]["batch"], x["inf"]["delta"]
    rng = np.random.default_rng(13)
    vals = rng.uniform(-1, 1, n)
    ct = D.encrypt(c, torch.tensor(vals, dtype=torch.float64, device="cuda"))
    refused = [
        lambda: c.rotationKeyGen([1]),
        lambda: c.evalSumKeyGen(),
        lambda: c.set_rotation_key(1, np.zeros((2, dn, 13 + len(p), N), np.uint64)),
        lambda: D.rotate(c, ct, 1),
        lambda: D.eval_sum(c, ct, 2),
        lambda: D.rotate(c, ct[:, :, :2].contiguous(), 1),  # at a level whose own T would fit: no key can exist
    ]
    for call in refused:
        with pytest.raises(ValueError, match="<= 16"):
            call()
        assert c.rotation_key_indices() == []
    same = D.rotate(c, ct, 0)
    assert same.data_ptr() != ct.data_ptr() and torch.equal(same, ct)
    assert torch.equal(D.eval_sum(c, ct, 1), ct)
    a, b = (_residue_batch(rng, q, 3, 13, N) for _ in range(2))
    a[0, 0, :, :4], b[0, 0, :, :4] = (q - 1)[:, None], (q - 1)[:, None]  # the largest sum
    assert np.array_equal(_u64(D.add(c, _dev(a), _dev(b))), (a + b) % q[:, None])
    two = D.add(c, ct, D.rotate(c, ct, 0))
    dec = D.decrypt(c, two, n, d).cpu().numpy()
    assert np.array_equal(dec, O.decrypt_vector(_u64(two), sk, q, psi, S, d, n))
    assert np.abs(dec - 2 * vals).max() < 1e-7
