"""Conjugation on the MI355X: the automorphism g = 2N - 1 through the rotation path.
Every residue bit-exact against tests/complex_ref.py's conj_ref (tests/rotation_ref.py's sigma_eval around
the oracle's EvalMult as the key switch; checked for meaning by tests/test_complex_ref.py) under the key read
back from the device, whose structure is checked exactly as tests/test_gpu_rotate.py checks a rotation key's.
Every output buffer starts filled with ones."""
import functools

import numpy as np
import pytest

import complex_ref as X
import dot_ref as DR
import dotp_ref as PJ
import rotation_ref as R
from conftest import set_switch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

# id -> (log2 ring, towers): the L = 4 chain on 2^12 (every level: three digits down to one tower), 2^13 / L3
# (the chunk split), and the two rings where g e wraps 32 bits (g = 2N - 1 >= 2^17, e < 2N)
CASES = {"n12_L4": (12, 4), "n13_L3": (13, 3), "n16_L2": (16, 2), "n17_L2": (17, 2)}


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _make(logn, L, seed, packing="complex"):
    c = m.CKKS("ckks", 1 << (logn - 1), 52, "", multDepth=L - 1, ringDim=1 << logn, seed=seed, decodeNoise=False,
               slotPacking=packing)
    assert c.genCryptoContextAndKeyGen() == 1
    return c


@functools.lru_cache(maxsize=None)
def ctx(cid):
    logn, L = CASES[cid]
    seed = 2100 + sorted(CASES).index(cid)
    c = _make(logn, L, seed)
    inf = c.info()
    assert (inf["ring_dim"], inf["num_towers"]) == (1 << logn, L)
    c.conjugateKeyGen()
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    pk, sk = c.get_keys()
    V = inf["values_per_ct"]
    v = np.random.default_rng(seed).uniform(-1, 1, 3 * V)
    ct = D.encrypt(c, torch.from_numpy(v).cuda())
    return dict(c=c, seed=seed, inf=inf, q=q, psi=psi, sk=sk, pk=pk, N=1 << logn, L=L, S=inf["batch"], V=V, v=v,
                ct=ct, ct_np=_u64(ct), key=c.get_conjugation_key(), d=inf["delta"])


def _conj(x, ct):
    out = torch.ones_like(ct)
    assert D.conj(x["c"], ct, out=out) is out
    return out


@pytest.mark.parametrize("cid", ["n12_L4", "n16_L2"])
def test_conjugation_key_structure(cid):
    """b + a s - [t in digit j] P sigma_g(s) is one small nonzero integer polynomial e_j in every tower of
    Q u P; its a is shared with no rotation key and not with the EvalMult key; the same seed gives the same
    key; it is one of the 64 and is dropped with them."""
    x = ctx(cid)
    c, key, N = x["c"], x["key"], x["N"]
    c.evalMultKeyGen()
    c.rotationKeyGen([1])
    evk, rk = c.get_eval_key(), c.get_rotation_key(1)
    assert key.shape == evk.shape
    e = X.key_error_g(key, X.conj_galois(N), x["sk"], x["q"], x["psi"])
    assert (e == e[:, :1]).all()
    assert np.abs(e).max() < 64 and all(e[j].any() for j in range(e.shape[0]))
    for other in (evk, rk):
        assert not (key[1] == other[1]).all(axis=-1).any()
    assert sorted(c.rotation_key_indices()) == [0, 1]  # the conjugation key is listed as index 0
    twin = _make(*CASES[cid], x["seed"])
    twin.conjugateKeyGen()
    assert np.array_equal(twin.get_conjugation_key(), key)
    c.conjugateKeyGen()  # again: the same key
    assert np.array_equal(c.get_conjugation_key(), key)


@pytest.mark.parametrize("l", [4, 3, 2, 1])
def test_conj_bitexact_at_every_level(l):
    x = ctx("n12_L4")
    ct = x["ct"][:, :, :l].contiguous()
    ref = X.conj_ref(_u64(ct), x["key"], x["q"], x["psi"])
    got = _conj(x, ct)  # K = 3
    assert np.array_equal(_u64(got), ref)
    assert np.array_equal(_u64(_conj(x, ct[:1].contiguous())), ref[:1])  # K = 1
    dec = D.decrypt(x["c"], got, 3 * x["V"], x["d"]).cpu().numpy()
    exp = x["v"].copy()
    exp[1::2] = -exp[1::2]
    err = np.abs(dec - exp).max()
    print("conj at %d towers: max error %.3g" % (l, err))
    assert err < 1e-7


@pytest.mark.parametrize("cid", ["n16_L2", "n17_L2"])
def test_conj_bitexact_where_the_index_product_wraps(cid):
    x = ctx(cid)
    for K in (1, 3):
        ct = x["ct"][:K].contiguous()
        assert np.array_equal(_u64(_conj(x, ct)), X.conj_ref(_u64(ct), x["key"], x["q"], x["psi"])), K


@pytest.mark.parametrize("logn", range(11, 18))
def test_pure_gather(logn):
    """c1 = 0: KeySwitch(sigma_g(0)) = 0 under any key, so conj((c0, 0)) = (c0[..., src], 0) with
    R.gather_index(N, 2N - 1)."""
    cid = {12: "n12_L4", 13: "n13_L3", 16: "n16_L2", 17: "n17_L2"}.get(logn)
    if cid:
        c, q = ctx(cid)["c"], ctx(cid)["q"]
    else:
        c = _make(logn, 2, 2200 + logn)
        c.conjugateKeyGen()
        q = np.array(c.info()["moduli"], np.uint64)
    N, L = 1 << logn, len(q)
    rng = np.random.default_rng(logn)
    ct = np.zeros((2, 2, L, N), np.uint64)
    for t in range(L):
        ct[:, 0, t] = rng.integers(0, int(q[t]), (2, N), dtype=np.uint64)
    out = torch.ones((2, 2, L, N), dtype=torch.int64, device="cuda")
    D.conj(c, _dev(ct), out=out)
    got = _u64(out)
    src = R.gather_index(N, X.conj_galois(N))
    assert not got[:, 1].any()
    assert np.array_equal(got[:, 0], ct[:, 0][..., src])


def test_chunk_split(monkeypatch):
    """SHELFI_EVAL_CHUNK_MIB = 1 at 2^13 / L3 (1.81 MiB of key-switch scratch a ciphertext,
    tests/test_gpu_eval_chunks.py): one ciphertext a chain, the same bits."""
    x = ctx("n13_L3")
    c = x["c"]
    one = _conj(x, x["ct"])
    assert c.eval_chunk_count() == 1
    assert np.array_equal(_u64(one), X.conj_ref(x["ct_np"], x["key"], x["q"], x["psi"]))
    set_switch(monkeypatch, "SHELFI_EVAL_CHUNK_MIB", "1")
    split = _conj(x, x["ct"])
    assert c.eval_chunk_count() == 3 > 1
    assert torch.equal(split, one)


def test_guards_and_key_exchange():
    x = ctx("n13_L3")
    c, ct, N = x["c"], x["ct"], x["N"]
    other = _make(*CASES["n13_L3"], 77)
    other.set_keys(x["pk"], x["sk"])
    with pytest.raises(RuntimeError, match="no conjugation key"):
        D.conj(other, ct)
    with pytest.raises(RuntimeError, match="no conjugation key"):
        other.get_conjugation_key()
    other.set_conjugation_key(x["key"])  # a keyless server is handed the key
    assert other.rotation_key_indices() == [0]
    assert torch.equal(D.conj(other, ct), D.conj(c, ct))
    bad = x["key"].copy()
    bad[0, 0, 0, 0] = x["q"][0]
    with pytest.raises(RuntimeError, match="residue"):
        other.set_conjugation_key(bad)
    with pytest.raises(ValueError):
        other.set_conjugation_key(bad[:1])
    assert other.genCryptoContextAndKeyGen() == 1  # new keys: dropped with the rotation keys
    with pytest.raises(RuntimeError, match="no conjugation key"):
        D.conj(other, ct)
    # overlap: the output on the input, and shifted over it
    with pytest.raises(ValueError, match="overlap"):
        D.conj(c, ct, out=ct)
    flat = torch.ones(ct.numel() + N, dtype=ct.dtype, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        D.conj(c, flat[N:].view(ct.shape), out=flat[:ct.numel()].view(ct.shape))
    lib = _lib.load()
    out = torch.ones_like(ct)
    for towers in (0, x["L"] + 1):
        assert lib.shelfi_dev_conjugate(c._ctx, ct.data_ptr(), 1, towers, out.data_ptr(), None) == _lib.SHELFI_ERR_ARG
    assert (out == 1).all()
    # the 64-key limit counts it
    many = _make(11, 2, 78)
    many.rotationKeyGen(range(1, 65))
    with pytest.raises(ValueError, match="64"):
        many.conjugateKeyGen()


def test_norm_is_dot_with_the_conjugate():
    """Under complex packing dot(u, conj(u)) holds sum_k |z_k[s]|^2 in slot s: bit-exact against dot_ref over
    conj_ref, and after rescale and eval_sum the decoded real part is sum (a^2 + b^2) over all 8192 values, at
    tests/test_gpu_dot.py's tolerance for its decoded inner product (1e-6, the same ring, chain and count)."""
    c = _make(12, 3, 2301)
    c.evalMultKeyGen()
    c.evalSumKeyGen()
    c.conjugateKeyGen()
    inf = c.info()
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    S, V, N = inf["batch"], inf["values_per_ct"], inf["ring_dim"]
    K = 2
    v = np.random.default_rng(12).uniform(-1, 1, K * V)
    assert v.size == 8192
    u = D.encrypt(c, torch.from_numpy(v).cuda())
    cu = D.conj(c, u)
    out = torch.ones((1, 2, 3, N), dtype=torch.int64, device="cuda")
    D.dot(c, u, cu, out=out)
    cref = X.conj_ref(_u64(u), c.get_conjugation_key(), q, psi)
    assert np.array_equal(_u64(cu), cref)
    assert np.array_equal(_u64(out), DR.dot_ref(_u64(u), cref, c.get_eval_key(), q, psi))
    scale = inf["delta"] * inf["delta"] / float(q[2])
    tot = D.eval_sum(c, D.rescale(c, out), S)
    dec = D.decrypt(c, tot, V, scale).cpu().numpy()
    exp = float(np.dot(v, v))
    err_re, err_im = np.abs(dec[0::2] - exp).max(), np.abs(dec[1::2]).max()
    print("sum |z|^2 = %.6f: real part error %.3g, imaginary part %.3g" % (exp, err_re, err_im))
    assert err_re < 1e-6 and err_im < 1e-6


def test_pack_slots_opens_the_norms_under_complex_packing():
    """INTEGRATION.md's recipe to its end: the norms of three complex-packed updates (dot with the conjugate,
    rescale, eval_sum) packed into ONE ciphertext and opened with one decrypt.  The one-hot plaintexts are the
    same in either packing (a 1.0 in the real part of slot p), so the packed ciphertext is tests/dotp_ref.py's
    pack_ref bit for bit, in complex mode, in real mode after it on the same context (the cached plaintexts), and
    on a context that packs in real mode first.  The decoded norms at tests/test_gpu_dot.py's 1e-6."""
    x = ctx("n12_L4")
    c, q, psi, N, S, V = x["c"], x["q"], x["psi"], x["N"], x["S"], x["V"]
    c.evalMultKeyGen()
    c.evalSumKeyGen()
    u = [x["ct"][k:k + 1].contiguous() for k in range(3)]
    tot = torch.cat([D.eval_sum(c, D.rescale(c, D.dot(c, uk, D.conj(c, uk))), S) for uk in u])
    assert tot.shape == (3, 2, 3, N)
    ref = PJ.pack_ref(_u64(tot), S, q, psi)
    out = torch.ones((1, 2, 2, N), dtype=torch.int64, device="cuda")
    assert D.pack_slots(c, tot, out=out) is out
    assert np.array_equal(_u64(out), ref)
    scale = x["d"] * x["d"] / float(q[3])
    dec = D.decrypt(c, out, V, scale).cpu().numpy()
    exp = np.array([np.dot(x["v"][k * V:(k + 1) * V], x["v"][k * V:(k + 1) * V]) for k in range(3)])
    e_norm = float(np.abs(dec[0:6:2] - exp).max())
    rest = float(max(np.abs(dec[1::2]).max(), np.abs(dec[6::2]).max()))
    print("packed norms: error %.3g, the other values %.3g" % (e_norm, rest))
    assert e_norm < 1e-6 and rest < 1e-6
    try:
        c.set_slot_packing("real")
        assert np.array_equal(_u64(D.pack_slots(c, tot)), ref)
    finally:
        c.set_slot_packing("complex")
    other = _make(12, 4, 79, packing="real")  # pack_slots needs no key
    assert np.array_equal(_u64(D.pack_slots(other, tot)), ref)
    other.set_slot_packing("complex")
    assert np.array_equal(_u64(D.pack_slots(other, tot)), ref)
    assert np.array_equal(_u64(D.pack_slots(other, tot[:2].contiguous())), PJ.pack_ref(_u64(tot[:2]), S, q, psi))
