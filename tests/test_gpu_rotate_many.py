"""Hoisted rotations (rotate_many) and the baby-step / giant-step linear transform on the MI355X.

rotate_many: every residue of every out[r] equal to tests/hoist_ref.py (decompose once, sigma_g as a gather of the
digits, inner product, ModDown; held to the oracle by tests/test_hoist_ref.py) under the rotation keys read back
from the device, and the decrypted slots equal to the rolled plaintext within tests/test_gpu_rotate.py's rule.
The contexts are that module's eight (one NTT block; alpha = 1; a partial last digit; two and three digits;
2^12-element blocks, where g e wraps 32 bits; 30-bit primes; sparse packing), the long chains A and C of
tests/test_gpu_rotate_edges.py with f4_cases' edge operands, and tests/test_gpu_eval_chunks.py's shape for the
chunk seams.  Every output buffer starts filled with ones.

lin_transform: a dense matrix and a band on a 16-slot context, against M @ x."""
import ctypes
import functools

import numpy as np
import pytest

import hoist_ref as H
from conftest import set_switch
from f4_cases import _full_batch, _planted_c2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

import test_gpu_rotate as TR  # noqa: E402  (the context table, ctx(), _key(), _decrypt())
import test_gpu_rotate_edges as TE  # noqa: E402  (chains A and C, chain(), _make())

_u64, _dev = TR._u64, TR._dev
# a single rotation; three; a zero, a repeat, and block-permuting and block-preserving g mixed
LISTS = {"one": ("1",), "three": ("1", "-1", "-2"), "mixed": ("0", "1", "1", "batch-1", "-1")}
LEVELS = [(cid, l) for cid in TR.LEVEL_IDS for l in range(1, TR.CASES[TR.IDS.index(cid)][1] + 2)]
EDGE_LEVELS = [(cid, Ll) for cid in ("A", "C") for Ll in TE.CHAINS[cid][5]]


def _ones(R, ct):
    K, _, l, N = ct.shape
    return torch.ones((R, K, 2, l, N), dtype=ct.dtype, device=ct.device)


def _indices(x, names):
    return [TR._index(x, n) for n in names]


@functools.lru_cache(maxsize=None)
def _refs(cid):
    """hoist_ref's rotations of the context's three ciphertexts by every index the lists use, computed once for
    all the cases of a context and never written to: {index: [3][2][L][N]}."""
    x = TR.ctx(cid)
    rs = sorted({r for names in LISTS.values() for r in _indices(x, names)})
    out = H.hoisted_ref(x["ct_np"], rs, {r: TR._key(x, r) for r in rs if r}, x["q"], x["psi"])
    out.setflags(write=False)
    return dict(zip(rs, out))


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("names", list(LISTS))
@pytest.mark.parametrize("cid", TR.IDS)
def test_rotate_many_bitexact_and_values(cid, names, K):
    x = TR.ctx(cid)
    c = x["c"]
    rs = _indices(x, LISTS[names])
    ct = x["ct"][:K].contiguous()
    out = _ones(len(rs), ct)
    got = D.rotate_many(c, ct, rs, out=out)
    assert got is out and c.eval_chunk_count() == 1
    ref = np.stack([_refs(cid)[r][:K] for r in rs])
    assert np.array_equal(_u64(got), ref)
    for i, r in enumerate(rs):
        err = np.abs(TR._decrypt(x, got[i]) - np.roll(x["x"][:K], -r, axis=1)).max()
        print("rotate_many %s r=%d: max error %.3g" % (cid, r, err))
        assert err < x["tol"]


# nine distinct non-zero indices in one call: more rotations than one workgroup pass serves, so the inner product
# runs in slices (blockIdx.y > 0, accumulator sets r >= 4); SHELFI_HOIST_KEYS_PER_PASS = 1 and 2 cut it into nine
# and five slices, 16 into one.  n15_L4: the compile-time kernel; n11_L2 and n17_L2: the runtime one.
NINE = (1, -1, -2, 2, 3, -3, 4, 5, 7)


@functools.lru_cache(maxsize=None)
def _nine(cid):
    """A context of its own under the shared one's key pair (the shared contexts' key lists are part of other
    tests' guards), with the nine keys, and the reference for two of the shared ciphertexts."""
    x = TR.ctx(cid)
    c = TR._make(x["case"], 700 + TR.IDS.index(cid))
    c.set_keys(*x["c"].get_keys())
    c.rotationKeyGen(NINE)
    ref = H.hoisted_ref(x["ct_np"][:2], NINE, {r: c.get_rotation_key(r) for r in NINE}, x["q"], x["psi"])
    ref.setflags(write=False)
    return c, ref


@pytest.mark.parametrize("per", [None, "1", "2", "16"])
@pytest.mark.parametrize("cid", ["n15_L4", "n11_L2", "n17_L2"])
def test_rotate_many_nine_rotations_at_every_group_size(monkeypatch, cid, per):
    x = TR.ctx(cid)
    c, ref = _nine(cid)
    set_switch(monkeypatch, "SHELFI_HOIST_KEYS_PER_PASS", per)
    ct = x["ct"][:2].contiguous()
    got = D.rotate_many(c, ct, NINE, out=_ones(9, ct))
    assert np.array_equal(_u64(got), ref)


@pytest.mark.parametrize("cid,l", LEVELS)
def test_rotate_many_at_every_level(cid, l):
    """A ciphertext truncated to l towers (fewer digits, the partial last digit, one tower)."""
    x = TR.ctx(cid)
    ct = x["ct"][:1, :, :l].contiguous()
    rs = [1, -2]
    ref = H.hoisted_ref(_u64(ct), rs, {r: TR._key(x, r) for r in rs}, x["q"], x["psi"])
    got = D.rotate_many(x["c"], ct, rs, out=_ones(2, ct))
    assert np.array_equal(_u64(got), ref)
    for i, r in enumerate(rs):
        assert np.abs(TR._decrypt(x, got[i]) - np.roll(x["x"][:1], -r, axis=1)).max() < x["tol"]


def _edge_ct(x, cid, Ll):
    """f4_cases' edge batch [K][2][Ll][N]: the decomposition sees c1 itself, so the planted polynomial (whole digits
    at 0, 1 and Q_j - 1) is c1 as it stands.  K = 3: all q_t - 1 in both components; c0 = 0 beside c1 all q_t - 1;
    the planted one.  K = 1: the planted one alone."""
    q, N = x["q"], x["N"]
    rng = np.random.default_rng([len(cid), ord(cid[0]), Ll, 21])
    pa, _, _ = _planted_c2(rng, q, x["psi"], Ll, x["alpha"], N)
    if x["K"] == 1:
        return pa[None].copy()
    return np.concatenate([_full_batch(q, 1, Ll, N), _full_batch(q, 1, Ll, N, poly0=0), pa[None]])


@pytest.mark.parametrize("cid,Ll", EDGE_LEVELS, ids=str)
def test_rotate_many_edges_on_long_chains(cid, Ll):
    """alpha 3 / kP 3 (the unfused ModUp and ModDown) and 12 towers with T = 16 and three digits, at their levels."""
    x = TE.chain(cid)
    ct = _edge_ct(x, cid, Ll)
    rs = [1, -2]
    dct = _dev(ct)
    got = _u64(D.rotate_many(x["c"], dct, rs, out=_ones(2, dct)))
    assert np.array_equal(got, H.hoisted_ref(ct, rs, x["keys"], x["q"], x["psi"]))


# ---- chunk seams: ring 2^13, 3 towers (dnum 2 / alpha 2 / kP 2), K = 5, R = 3 ----
# a ciphertext's scratch: d2e | d2c | ext = (3 + 3 + 7) N 8 = 832 KiB shared, accQ | accP | z = (6 + 4 + 6) N 8 =
# 1 MiB per rotation in flight.  8 MiB: all three rotations in flight, two ciphertexts a chain -- chains of 2, 2, 1.
# 2 MiB: one ciphertext's decomposition leaves room for ONE accumulator set, so the call also splits over three
# rotation groups: 5 chains x 3 groups.
@pytest.mark.parametrize("mib,chains", [("8", 3), ("2", 15)])
def test_chunked_rotate_many_is_counted_and_bit_identical(monkeypatch, mib, chains):
    import test_gpu_eval_chunks as TC

    x = TC.ctx()
    c, ct = x["c"], x["ct"]
    rs = [1, -2, 2]
    c.rotationKeyGen(rs)
    set_switch(monkeypatch, TC.SWITCH, None)
    whole = D.rotate_many(c, ct, rs, out=_ones(3, ct))
    assert c.eval_chunk_count() == 1
    set_switch(monkeypatch, TC.SWITCH, mib)
    got = D.rotate_many(c, ct, rs, out=_ones(3, ct))
    print("rotate_many under %s MiB: %d chains" % (mib, c.eval_chunk_count()))
    assert c.eval_chunk_count() == chains > 1
    assert torch.equal(got, whole)
    ref = H.hoisted_ref(x["ct_np"][3:], rs, {r: c.get_rotation_key(r) for r in rs}, x["q"], x["psi"])
    assert np.array_equal(_u64(got)[:, 3:], ref)  # the ragged last chain (and its neighbour) against the reference


def test_imported_keys_give_identical_rotations():
    x = TR.ctx("n13_L3")
    c = x["c"]
    other = TR._make(x["case"], 98)
    other.set_keys(*c.get_keys())
    rs = [1, -2, 1]
    with pytest.raises(RuntimeError, match="rotation key"):
        D.rotate_many(other, x["ct"], rs)
    for r in (1, -2):
        other.set_rotation_key(r, TR._key(x, r))
    assert torch.equal(D.rotate_many(other, x["ct"], rs), D.rotate_many(c, x["ct"], rs))


def test_guards():
    x = TR.ctx("n11_L2")
    c, ct, S = x["c"], x["ct"], x["S"]
    L, N = len(x["q"]), x["inf"]["ring_dim"]
    lib = _lib.load()
    ones = _ones(2, ct)
    # a missing key: every key is looked up before anything is enqueued
    with pytest.raises(RuntimeError, match="no rotation key for index 3"):
        D.rotate_many(c, ct, [1, 3], out=ones)
    assert bool((ones == 1).all())
    # overlap: the output on the input, and the input inside a later out[r]
    flat = torch.empty(3 * ct.numel(), dtype=ct.dtype, device="cuda")
    for at in (0, ct.numel(), 2 * ct.numel() - N):
        src = flat[at:at + ct.numel()].view(ct.shape)
        with pytest.raises(ValueError, match="overlap"):
            D.rotate_many(c, src, [1, -1], out=flat[:2 * ct.numel()].view((2,) + tuple(ct.shape)))
    # R = 0 and R = 65: the wrapper's check and the C ABI's own; R = 0 and K = 0 enqueue nothing
    for rs in ([], [1] * 65):
        with pytest.raises(ValueError):
            D.rotate_many(c, ct, rs)
    idx = (ctypes.c_int32 * 65)(*([1] * 65))
    big = torch.ones((2,) + tuple(ct.shape), dtype=ct.dtype, device="cuda")
    D.rotate(c, ct, 1)
    assert c.eval_chunk_count() == 1
    assert lib.shelfi_dev_rotate_many(c._ctx, ct.data_ptr(), 3, L, idx, 0, big.data_ptr(), None) == 0
    assert c.eval_chunk_count() == 0 and bool((big == 1).all())
    D.rotate(c, ct, 1)
    assert lib.shelfi_dev_rotate_many(c._ctx, ct.data_ptr(), 0, L, idx, 2, big.data_ptr(), None) == 0
    assert c.eval_chunk_count() == 0 and bool((big == 1).all())
    assert lib.shelfi_dev_rotate_many(c._ctx, ct.data_ptr(), 1, L, idx, 65, big.data_ptr(), None) == _lib.SHELFI_ERR_ARG
    # NULL pointers, towers outside 1..L
    assert lib.shelfi_dev_rotate_many(c._ctx, None, 1, L, idx, 2, big.data_ptr(), None) == _lib.SHELFI_ERR_ARG
    assert lib.shelfi_dev_rotate_many(c._ctx, ct.data_ptr(), 1, L, None, 2, big.data_ptr(), None) == _lib.SHELFI_ERR_ARG
    assert lib.shelfi_dev_rotate_many(c._ctx, ct.data_ptr(), 1, L, idx, 2, None, None) == _lib.SHELFI_ERR_ARG
    for towers in (0, L + 1):
        assert lib.shelfi_dev_rotate_many(c._ctx, ct.data_ptr(), 1, towers, idx, 2, big.data_ptr(),
                                          None) == _lib.SHELFI_ERR_ARG
    with pytest.raises(ValueError):
        D.rotate_many(c, torch.empty((1, 2, L + 1, N), dtype=ct.dtype, device="cuda"), [1])
    # |index| = batch
    for r in (S, -S):
        with pytest.raises(ValueError, match="batch"):
            D.rotate_many(c, ct, [1, r], out=ones)
    assert bool((ones == 1).all()) and bool((big == 1).all())


def test_chain_too_long_for_key_switching():
    """13 towers need 5 special primes: 18 towers exceed the 16 the kernels hold.  The call says so, before it looks
    for keys the context can never hold -- also at a level whose own T would fit; a list of zeros needs no key."""
    x = TE._make(1 << 12, 13, 52, 60, 1214)
    c = x["c"]
    vals = np.random.default_rng(14).uniform(-1, 1, x["inf"]["batch"])
    ct = D.encrypt(c, torch.tensor(vals, dtype=torch.float64, device="cuda"))
    for call in (lambda: D.rotate_many(c, ct, [0, 1]), lambda: D.rotate_many(c, ct[:, :, :2].contiguous(), [1])):
        with pytest.raises(ValueError, match="<= 16"):
            call()
    same = D.rotate_many(c, ct, [0, 0])
    assert torch.equal(same[0], ct) and torch.equal(same[1], ct)


# ---- lin_transform: 16 slots on ring 2^11, 3 towers ----
BATCH = 16


def _lin_ctx(seed):
    c = m.CKKS("ckks", BATCH, 52, "", multDepth=2, firstModBits=60, ringDim=2048, seed=seed, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    assert (inf["batch"], inf["ring_dim"], inf["num_towers"]) == (BATCH, 2048, 3)
    return c, inf


def _band():
    rng = np.random.default_rng(32)
    M = np.zeros((BATCH, BATCH))
    s = np.arange(BATCH)
    for d in (-1, 0, 1):
        M[s, (s + d) % BATCH] = rng.uniform(-1, 1, BATCH)
    return M


@pytest.mark.parametrize("name,babies,keys", [("dense", 4, [1, 2, 3, 4, 8, 12]), ("band", None, [-2, 1])])
def test_lin_transform_matches_the_matrix_product(name, babies, keys):
    """y = M x within (d + 1) tol for d diagonals: each rotated term carries at most tol (tests/test_gpu_rotate.py's
    rule), the entries are at most 1 in magnitude, and there is one rescale.  Only the keys lin_transform_indices
    lists are generated."""
    c, inf = _lin_ctx(40 + len(name))
    M = np.random.default_rng(31).uniform(-1, 1, (BATCH, BATCH)) if name == "dense" else _band()
    diags = D.diagonals(M)
    assert len(diags) == (BATCH if name == "dense" else 3)
    assert D.lin_transform_indices(diags, babies) == keys
    c.rotationKeyGen(keys)
    assert sorted(c.rotation_key_indices()) == keys
    K = 2
    xs = np.random.default_rng(33).uniform(-1, 1, (K, BATCH))
    ct = D.encrypt(c, torch.tensor(xs.ravel(), dtype=torch.float64, device="cuda"))
    y = D.lin_transform(c, ct, diags, babies=babies)
    assert tuple(y.shape) == (K, 2, 2, 2048)  # one tower fewer, at the input's scale
    dec = D.decrypt(c, y, K * BATCH, inf["delta"]).cpu().numpy().reshape(K, BATCH)
    err = np.abs(dec - xs @ M.T).max()
    tol = max(1e-7, 2.0 ** (18 - 52))
    print("lin_transform %s: %d diagonals, max error %.3g (bound %.3g)" % (name, len(diags), err, (len(diags) + 1) * tol))
    assert err < (len(diags) + 1) * tol
