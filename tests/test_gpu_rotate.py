"""Slot rotations, EvalSum and the plain ciphertext add on the MI355X: every residue
bit-exact against tests/rotation_ref.py (the oracle's NTTs around the coefficient-domain automorphism,
and its EvalMult as the key switch; checked for meaning by tests/test_rotation_ref.py), under the
rotation keys read back from the device, whose structure is checked exactly; and the decrypted slots
equal to the rolled / summed plaintext within tests/test_gpu_f4.py's tolerance rule.

Contexts: tests/test_gpu_f4.py's seven (one NTT block; alpha = 1; a partial last digit; two and three
full digits; 2^12-element blocks; 30-bit scaling primes) and a sparsely packed one (ring 2^15, batch
4096).  Whether PALISADE permutes before or after switching is unpinned: there is no rotated fixture."""
import functools

import numpy as np
import pytest

import oracle as O
import rotation_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

# (batch, multDepth, scaleBits, firstModBits[, ringDim]); the last is the sparse context.  The 2^11
# ring is asked for by name: ParamsGen's own choice for batch 1024 is 2^13, which has a columns pass.
CASES = [(4096, 1, 52, 60), (4096, 2, 52, 60, 8192), (16384, 3, 52, 60), (32768, 5, 52, 60),
         (1024, 1, 52, 60, 2048), (65536, 1, 52, 60), (4096, 1, 30, 40), (4096, 3, 52, 60)]
IDS = ["n13_L2", "n13_L3", "n15_L4", "n16_L6", "n11_L2", "n17_L2", "n13_30bit", "n15_sparse"]
SUM_IDS = ("n11_L2", "n13_L3", "n15_sparse")  # EvalSum and the composed circuit
LEVEL_IDS = ("n15_L4", "n16_L6")  # every number of towers
ROTS = ("1", "-1", "-2", "batch-1")


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _make(case, seed):
    batch, depth, sb, fb = case[:4]
    rd = case[4] if len(case) > 4 else 0
    c = m.CKKS("ckks", batch, sb, "", multDepth=depth, firstModBits=fb, ringDim=rd, seed=seed, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    return c


@functools.lru_cache(maxsize=None)
def ctx(cid):
    """One context per case for the whole module: keys, three ciphertexts of uniform slots."""
    case = CASES[IDS.index(cid)]
    seed = 500 + IDS.index(cid)
    c = _make(case, seed)
    inf = c.info()
    S = inf["batch"]
    assert (cid != "n15_sparse") == (S == inf["ring_dim"] // 2)
    c.rotationKeyGen([1, -1, -2, S - 1, 0])
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    pk, sk = c.get_keys()
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, 3 * S)
    ct = D.encrypt(c, torch.tensor(x, dtype=torch.float64, device="cuda"))
    tol = max(1e-7, 2.0 ** (18 - case[2]))  # tests/test_gpu_f4.py's rule (value check only)
    return dict(c=c, case=case, seed=seed, inf=inf, S=S, q=q, psi=psi, sk=sk, x=x.reshape(3, S), ct=ct,
                ct_np=_u64(ct), tol=tol, d=inf["delta"], keys={})


def _key(x, r):
    if r not in x["keys"]:
        x["keys"][r] = x["c"].get_rotation_key(r)
    return x["keys"][r]


def _index(x, name):
    return x["S"] - 1 if name == "batch-1" else int(name)


def _decrypt(x, ct, scale=None):
    l = ct.shape[2]
    n = ct.shape[0] * x["S"]
    scale = x["d"] if scale is None else scale
    dec = D.decrypt(x["c"], ct, n, scale).cpu().numpy()
    ref = O.decrypt_vector(_u64(ct), x["sk"][:l], x["q"][:l], x["psi"][:l], x["S"], scale, n)
    assert np.array_equal(dec, ref)
    return dec.reshape(-1, x["S"])


@pytest.mark.parametrize("cid", IDS)
def test_rotation_key_structure(cid):
    """b + a s - [t in digit j] P sigma_g(s) is one small nonzero integer polynomial e_j in every tower
    of Q u P (|e| < 64, the oracle's CDT buffer); no a is shared between two indices or with the EvalMult
    key; the same seed gives the same keys."""
    x = ctx(cid)
    c, S = x["c"], x["S"]
    c.rotationKeyGen([S // 2])
    c.evalMultKeyGen()
    evk = c.get_eval_key()
    # keys are held by Galois element: at full packing -1 and batch - 1 are one key
    ring = x["inf"]["ring_dim"]
    held = {R.galois(ring, r) for r in c.rotation_key_indices()}
    assert held >= {R.galois(ring, r) for r in (1, -1, -2, S - 1, S // 2)} and 1 not in held
    keys = {r: _key(x, r) for r in (1, -2, S // 2)}
    for r, key in keys.items():
        assert key.shape == evk.shape
        e = R.key_error(key, r, x["sk"], x["q"], x["psi"])
        assert (e == e[:, :1]).all(), r
        assert np.abs(e).max() < 64 and all(e[j].any() for j in range(e.shape[0])), r
        assert not np.array_equal(key[1], evk[1])
        assert not (key[1] == evk[1]).all(axis=-1).any()
    assert not (keys[1][1] == keys[-2][1]).all(axis=-1).any()
    assert not (keys[1][1] == keys[S // 2][1]).all(axis=-1).any()
    twin = _make(x["case"], x["seed"])
    twin.rotationKeyGen([-2, 1])
    assert np.array_equal(twin.get_rotation_key(1), keys[1]) and np.array_equal(twin.get_rotation_key(-2), keys[-2])
    c.rotationKeyGen([1])  # a repeated index: the same key again
    assert np.array_equal(c.get_rotation_key(1), keys[1])


@pytest.mark.parametrize("name", ROTS)
@pytest.mark.parametrize("cid", IDS)
def test_rotate_bitexact_and_values(cid, name):
    x = ctx(cid)
    c, r = x["c"], _index(x, name)
    ref = R.rotate_ref(x["ct_np"], r, _key(x, r), x["q"], x["psi"])
    got = D.rotate(c, x["ct"], r)  # K = 3
    assert np.array_equal(_u64(got), ref)
    assert np.array_equal(_u64(D.rotate(c, x["ct"][:1], r)), ref[:1])  # K = 1
    dec = _decrypt(x, got)
    assert np.array_equal(dec.ravel(), O.decrypt_vector(ref, x["sk"], x["q"], x["psi"], x["S"], x["d"], 3 * x["S"]))
    err = np.abs(dec - np.roll(x["x"], -r, axis=1)).max()
    print("rotate %s r=%d: max error %.3g" % (cid, r, err))
    assert err < x["tol"]


@pytest.mark.parametrize("cid", IDS)
def test_round_trip_and_identity(cid):
    x = ctx(cid)
    c, ct = x["c"], x["ct"]
    back = D.rotate(c, D.rotate(c, ct, 1), -1)
    assert np.abs(_decrypt(x, back) - x["x"]).max() < x["tol"]
    same = D.rotate(c, ct, 0)
    assert same.data_ptr() != ct.data_ptr() and torch.equal(same, ct)
    assert D.rotate(c, ct, 0, out=ct) is ct and np.array_equal(_u64(ct), x["ct_np"])


@pytest.mark.parametrize("cid,l", [(cid, l) for cid in LEVEL_IDS for l in range(1, CASES[IDS.index(cid)][1] + 2)])
def test_rotate_at_every_level(cid, l):
    """A ciphertext truncated to l towers (fewer digits, the partial last digit, one tower)."""
    x = ctx(cid)
    ct = x["ct"][:1, :, :l].contiguous()
    ref = R.rotate_ref(_u64(ct), -2, _key(x, -2), x["q"], x["psi"])
    got = D.rotate(x["c"], ct, -2)
    assert np.array_equal(_u64(got), ref)
    assert np.abs(_decrypt(x, got) - np.roll(x["x"][:1], 2, axis=1)).max() < x["tol"]


def test_rotate_a_rescaled_product():
    """Rotation one level down, of a ciphertext that went through EvalMult and ModReduce."""
    x = ctx("n13_L3")
    c, q = x["c"], x["q"]
    c.evalMultKeyGen()
    sq = D.rescale(c, D.mult(c, x["ct"], x["ct"]))
    got = D.rotate(c, sq, 1)
    assert np.array_equal(_u64(got), R.rotate_ref(_u64(sq), 1, _key(x, 1), q, x["psi"]))
    dec = _decrypt(x, got, x["d"] * x["d"] / float(q[-1]))
    assert np.abs(dec - np.roll(x["x"] ** 2, -1, axis=1)).max() < x["tol"]


@functools.lru_cache(maxsize=None)
def _sum_keys(cid):
    x = ctx(cid)
    x["c"].evalSumKeyGen()
    return {1 << i: _key(x, 1 << i) for i in range(x["S"].bit_length() - 1)}


def _sliding(xs, n):
    return sum(np.roll(xs, -j, axis=1) for j in range(n))


@pytest.mark.parametrize("n", ["1", "4", "batch"])
@pytest.mark.parametrize("cid", SUM_IDS)
def test_eval_sum_bitexact_and_values(cid, n):
    x = ctx(cid)
    keys = _sum_keys(cid)
    n = x["S"] if n == "batch" else int(n)
    K = 1 if n == x["S"] else 3  # log2(batch) reference rotations: one ciphertext
    ct = x["ct"][:K].contiguous()
    got = D.eval_sum(x["c"], ct, n)
    assert np.array_equal(_u64(got), R.eval_sum_ref(_u64(ct), n, keys, x["q"], x["psi"]))
    exp = x["x"][:K].sum(axis=1, keepdims=True) if n == x["S"] else _sliding(x["x"][:K], n)
    err = np.abs(_decrypt(x, got) - exp).max()
    print("eval_sum %s n=%d: max error %.3g" % (cid, n, err))
    assert err < x["tol"] * n


@pytest.mark.parametrize("cid", SUM_IDS)
def test_squared_norm_of_an_encrypted_update(cid):
    """INTEGRATION.md's example: eval_sum(rescale(mult(ct, ct)), batch) holds sum x^2 in every slot.
    The slots are uniform in (-1/4, 1/4): on the L = 2 chain the result sits on one 60-bit tower at a
    52-bit scale, which holds |values| below 2^7 -- sum x^2 is about batch / 48 <= 86 here (with slots
    in (-1, 1) it is about 341 at batch 1024 and wraps)."""
    x = ctx(cid)
    c, S = x["c"], x["S"]
    _sum_keys(cid)
    c.evalMultKeyGen()
    y = x["x"] / 4
    ct = D.encrypt(c, torch.tensor(y.ravel(), dtype=torch.float64, device="cuda"))
    norm = D.eval_sum(c, D.rescale(c, D.mult(c, ct, ct)), S)
    dec = _decrypt(x, norm, x["d"] * x["d"] / float(x["q"][-1]))
    exp = (y ** 2).sum(axis=1, keepdims=True)
    err = np.abs(dec - exp).max()
    print("squared norm %s: max error %.3g" % (cid, err))
    assert err < x["tol"] * S


@pytest.mark.parametrize("cid", ["n11_L2", "n16_L6", "n13_30bit"])
def test_add(cid):
    x = ctx(cid)
    c, q = x["c"], x["q"]
    rng = np.random.default_rng(9)
    for l in (len(q), 1):
        a, b = (np.stack([rng.integers(0, int(q[t]), (3, 2, x["inf"]["ring_dim"]), dtype=np.uint64)
                          for t in range(l)], axis=2) for _ in range(2))
        a[0, 0, :, :4], b[0, 0, :, :4] = (q[:l] - 1)[:, None], (q[:l] - 1)[:, None]  # the largest sum
        ref = (a + b) % q[:l, None]
        ta, tb = _dev(a), _dev(b)
        assert np.array_equal(_u64(D.add(c, ta, tb)), ref)
        assert D.add(c, ta, tb, out=ta) is ta and np.array_equal(_u64(ta), ref) and np.array_equal(_u64(tb), b)
        ta = _dev(a)
        D.add(c, ta, tb, out=tb)
        assert np.array_equal(_u64(tb), ref)
    s2 = D.add(c, x["ct"], D.rotate(c, x["ct"], 1))
    assert np.abs(_decrypt(x, s2) - _sliding(x["x"], 2)).max() < 2 * x["tol"]
    with pytest.raises(ValueError):
        D.add(c, x["ct"], x["ct"][:1])
    flat = torch.zeros(x["ct"].numel() + 8, dtype=x["ct"].dtype, device="cuda")
    with pytest.raises(ValueError, match="overlap"):  # an output shifted over an input
        D.add(c, flat[8:].view(x["ct"].shape), x["ct"], out=flat[:x["ct"].numel()].view(x["ct"].shape))


def test_guards():
    x = ctx("n11_L2")
    c, ct, S = x["c"], x["ct"], x["S"]
    L, N = len(x["q"]), x["inf"]["ring_dim"]
    with pytest.raises(RuntimeError, match="rotation key"):
        D.rotate(c, ct, 3)
    with pytest.raises(RuntimeError, match="rotation key"):
        c.get_rotation_key(3)
    fresh = _make(x["case"], 77)
    fresh.rotationKeyGen([1])
    fct = D.encrypt(fresh, torch.tensor(x["x"][0], dtype=torch.float64, device="cuda"))
    D.rotate(fresh, fct, 1)
    assert fresh.genCryptoContextAndKeyGen() == 1  # new keys: the rotation keys are dropped
    assert fresh.rotation_key_indices() == []
    with pytest.raises(RuntimeError, match="rotation key"):
        D.rotate(fresh, fct, 1)
    with pytest.raises(RuntimeError, match="rotation key"):
        D.eval_sum(fresh, fct, 2)
    # overlap: the output on the input, and shifted over it
    with pytest.raises(ValueError, match="overlap"):
        D.rotate(c, ct, 1, out=ct)
    flat = torch.empty(ct.numel() + N, dtype=ct.dtype, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        D.rotate(c, flat[N:].view(ct.shape), 1, out=flat[:ct.numel()].view(ct.shape))
    with pytest.raises(ValueError, match="overlap"):
        D.eval_sum(c, flat[N:].view(ct.shape), 1, out=flat[:ct.numel()].view(ct.shape))
    # towers 0 or above L: the wrapper's shape check, and the C ABI's own
    with pytest.raises(ValueError):
        D.rotate(c, torch.empty((1, 2, L + 1, N), dtype=ct.dtype, device="cuda"), 1)
    lib = _lib.load()
    out = torch.empty_like(ct)
    for towers in (0, L + 1):
        assert lib.shelfi_dev_rotate(c._ctx, ct.data_ptr(), 1, towers, 1, out.data_ptr(), None) == _lib.SHELFI_ERR_ARG
        assert lib.shelfi_dev_eval_sum(c._ctx, ct.data_ptr(), 1, towers, 1, out.data_ptr(), None) == _lib.SHELFI_ERR_ARG
        assert lib.shelfi_dev_add(c._ctx, ct.data_ptr(), ct.data_ptr(), 1, towers, out.data_ptr(),
                                  None) == _lib.SHELFI_ERR_ARG
    for r in (S, -S):
        with pytest.raises(ValueError):
            D.rotate(c, ct, r)
        with pytest.raises(ValueError):
            c.rotationKeyGen([r])
    for n in (0, 3, 2 * S):
        with pytest.raises(ValueError):
            D.eval_sum(c, ct, n)
    # 64 keys at the most; a refused list leaves the keys held as they were
    many = _make(x["case"], 78)
    many.rotationKeyGen(range(1, 65))
    assert sorted(many.rotation_key_indices()) == list(range(1, 65))
    with pytest.raises(ValueError, match="64"):
        many.rotationKeyGen([65])
    with pytest.raises(ValueError, match="64"):
        many.set_rotation_key(65, many.get_rotation_key(1))
    many.rotationKeyGen([64, 0])  # held already / skipped
    assert len(many.rotation_key_indices()) == 64


def test_imported_key_gives_identical_rotations():
    x = ctx("n13_L3")
    c = x["c"]
    other = _make(x["case"], 99)
    other.set_keys(*c.get_keys())
    with pytest.raises(RuntimeError, match="rotation key"):
        D.rotate(other, x["ct"], -2)
    other.set_rotation_key(-2, _key(x, -2))
    assert other.rotation_key_indices() == [-2]
    assert torch.equal(D.rotate(other, x["ct"], -2), D.rotate(c, x["ct"], -2))
    bad = _key(x, -2).copy()
    bad[0, 0, 0, 0] = x["q"][0]  # a residue >= q
    with pytest.raises(RuntimeError, match="residue"):
        other.set_rotation_key(-2, bad)
    with pytest.raises(ValueError):
        other.set_rotation_key(-2, bad[:1])
