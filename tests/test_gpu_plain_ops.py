"""Plaintext operands on the MI355X: D.encode bit for bit against oracle.encode on
every ring, gap and tower class of tests/encode_edge_inputs.py, at the edge of its range and across a
chunk seam; D.mult_plain / add_plain / sub_plain / sub / neg bit for bit against tests/plain_ref.py
(checked for meaning on the CPU by tests/test_plain_ref.py) with planted edge residues; the decrypted
values; a context without keys; the composed distance circuit; the guards.

Tolerances of the value checks: tests/test_gpu_f4.py's rule max(1e-7, 2^(18 - scaleBits)) for anything
that went through a product and ModReduce, and for sums / differences of fresh ciphertexts (whose own
error is far below it).  The composed circuit's slot 0 is a sum of `batch` slot products, each within
that rule with independent errors: sqrt(batch) times the rule."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import encode_edge_inputs as E
import oracle as O
import plain_ref as P
from conftest import set_switch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

LEVEL_SHAPES = ("2^15/L4", "2^16/L2")  # every number of towers


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _x(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def bare(name):
    """A context of an encode_edge_inputs shape that never had keys; its chain is the oracle's."""
    batch, N, depth, sb, fb = E.SHAPES[name]
    ck = m.CKKS("ckks", batch, sb, "", multDepth=depth, firstModBits=fb, ringDim=N, seed=9, decodeNoise=False)
    ch = E.chain(name)
    inf = ck.info()
    assert not inf["keys_loaded"]
    assert (inf["ring_dim"], inf["batch"], inf["delta"]) == (ch.N, ch.S, ch.delta)
    assert np.array_equal(np.array(inf["moduli"], np.uint64), ch.q)
    assert np.array_equal(np.array(inf["roots"], np.uint64), ch.psi)
    return ck, ch


def _ref_encode(ch, x, towers=None, scale=None):
    towers = ch.L if towers is None else towers
    scale = ch.delta if scale is None else scale
    K = -(-len(x) // ch.S)
    return np.stack([O.encode(x[k * ch.S:(k + 1) * ch.S], ch.N, ch.S, scale, ch.q[:towers], ch.psi[:towers])
                     for k in range(K)])


def _encode(ck, x, **kw):
    pt = D.encode(ck, _x(x), **kw)
    assert pt.dtype == torch.int64
    return _u64(pt)


def _canonical(out, q):
    return all((out[..., t, :] < q[t]).all() for t in range(out.shape[-2]))


# ------------------------------------------------------------------ 1. encode ----
@pytest.mark.parametrize("name", list(E.SHAPES))
def test_encode_bitexact_on_every_shape(name):
    ck, ch = bare(name)
    x = np.random.default_rng(len(name)).uniform(-1, 1, 2 * ch.S + 5)  # K = 3, a partial last vector
    got = _encode(ck, x)
    assert got.shape == (3, ch.L, ch.N)
    assert np.array_equal(got, _ref_encode(ch, x))
    assert not _encode(ck, np.zeros(ch.S + 1)).any()


@pytest.mark.parametrize("name", LEVEL_SHAPES)
def test_encode_every_tower_count_and_scale(name):
    ck, ch = bare(name)
    x = np.random.default_rng(3).uniform(-1, 1, 2 * ch.S + 5)
    for towers in range(1, ch.L + 1):
        scale = float(int(ch.q[towers - 1]))
        got = _encode(ck, x, towers=towers, scale=scale)
        assert got.shape == (3, towers, ch.N)
        assert np.array_equal(got, _ref_encode(ch, x, towers, scale)), towers
    assert np.array_equal(_encode(ck, x, scale=2.0 ** 30), _ref_encode(ch, x, scale=2.0 ** 30))


@pytest.mark.parametrize("K,whole", [(1, None), (128, None), (128, "0")], ids=["K1", "K128", "K128_fft_passes"])
def test_encode_batch_sizes_at_the_metric_ring(K, whole, monkeypatch):
    """K = 128 takes the whole-vector FFT (kFftWholeMinK) unless SHELFI_FFT_WHOLE=0."""
    ck, ch = bare("2^15/L4")
    if whole is not None:
        set_switch(monkeypatch, "SHELFI_FFT_WHOLE", whole)
    x = np.random.default_rng(K).uniform(-1, 1, K * ch.S - 7)
    assert np.array_equal(_encode(ck, x), _ref_encode(ch, x))


# ------------------------------------------------------------- 2. range edge ----
@pytest.mark.parametrize("name", list(E.SHAPES))
def test_encode_range_edge(name):
    ck, ch = bare(name)
    good = np.random.default_rng(5).uniform(-1, 1, ch.S + 3)
    good_ref = _ref_encode(ch, good)

    def refused(x):
        with pytest.raises(ValueError):
            D.encode(ck, _x(x))
        # the flag word does not leak into the next call
        assert np.array_equal(_encode(ck, good), good_ref)

    band = E.dense_band(ch.S, ch.delta, 2)  # every coefficient about 0.99 2^61 |cos| or |sin|
    assert np.array_equal(_encode(ck, band), _ref_encode(ch, band))
    top = E.at_coefficient(ch.N, ch.S, ch.delta, "max_fast")
    assert top.coeff == 2 ** 61 and top.log_approx == 0
    for sign in (1.0, -1.0):
        x = E.constant(ch.S, sign * top.c)
        assert np.array_equal(_encode(ck, x), _ref_encode(ch, x))
    over = E.at_coefficient(ch.N, ch.S, ch.delta, "first_redo")
    assert over.c == np.nextafter(top.c, np.inf) and over.coeff > 2 ** 61
    refused(E.constant(ch.S, over.c))
    refused(np.concatenate([good[:ch.S], E.constant(ch.S, -over.c)]))  # the second plaintext of a call
    for bad in (np.nan, np.inf, -np.inf):
        x = good.copy()
        x[2] = bad
        refused(x)


# -------------------------------------------------------------- 3. chunk seam ----
def _chunks(K, S, mib):
    """dev_chunk over the documented scratch of one plaintext: 16 bytes per slot and 64 (shelfi.h)."""
    cap = max(1, (mib << 20) // (16 * S + 64))
    n = -(-K // cap)
    return n, -(-K // n)


def test_encode_chunk_seam(monkeypatch):
    """K = 5 at 2^13 / L2 fits one chunk even at the switch's finest setting (1 MiB holds 15 plaintexts'
    FFT buffers of 64 KiB, the encode's only scratch): it is run at that setting, and so is K = 17, which
    1 MiB splits in two (chunks of 9 and 8, the second starting inside x at a plaintext boundary)."""
    ck, ch = bare("2^13/L2")
    assert _chunks(5, ch.S, 1)[0] == 1 and _chunks(16, ch.S, 1)[0] == 2 and _chunks(17, ch.S, 1) == (2, 9)
    for K in (5, 17):
        x = np.random.default_rng(K).uniform(-1, 1, K * ch.S - 11)
        one = _encode(ck, x)
        set_switch(monkeypatch, "SHELFI_DEV_CHUNK_MIB", "1")
        two = _encode(ck, x)
        set_switch(monkeypatch, "SHELFI_DEV_CHUNK_MIB", None)
        assert np.array_equal(one, two)
        assert np.array_equal(one, _ref_encode(ch, x))


# ----------------------------------------------------------- 4. pointwise ----
POINT = ("2^11/L2", "30-bit", "2^15/L4", "2^17/L2")


def _planted(ch, towers, K=3, seed=0):
    """Random canonical ciphertexts a, b [K][2][towers][N] and plaintexts [K][towers][N] with the edge
    residues of plain_ref planted at both ends of every polynomial."""
    rng = np.random.default_rng(100 * towers + seed)

    def rand(*shape):
        out = np.empty(shape + (towers, ch.N), np.uint64)
        for t in range(towers):
            out[..., t, :] = rng.integers(0, int(ch.q[t]), shape + (ch.N,), dtype=np.uint64)
        return out

    a = P.plant(rand(K, 2), ch.q, P.CT_EDGES, div=4)
    b = P.plant(rand(K, 2), ch.q, P.CT_EDGES, div=2)
    pt = P.plant(rand(K), ch.q, P.PT_EDGES)
    return a, b, pt


def _check_lib(ck, t, towers, L):
    if towers == L:  # the entry point reads [K][2][L][N]
        rc = _lib.load().shelfi_dev_check_residues(ck._ctx, C.c_void_p(t.data_ptr()), t.shape[0], None)
        assert rc == 0


@pytest.mark.parametrize("name", POINT)
def test_pointwise_bitexact(name):
    ck, ch = bare(name)
    for towers in (range(1, ch.L + 1) if name == "2^15/L4" else (ch.L,)):
        a, b, pt = _planted(ch, towers)
        q = ch.q
        A, B = _dev(a), _dev(b)
        for fn, ref in ((D.mult_plain, P.mult_plain), (D.add_plain, P.add_plain), (D.sub_plain, P.sub_plain)):
            exp_k, exp_1 = ref(a, pt, q), ref(a, pt[:1], q)
            # Kp = K, Kp = 1, and the [towers][N] form of Kp = 1
            for p, exp in ((pt, exp_k), (pt[:1], exp_1), (pt[0], exp_1)):
                out = fn(ck, A, _dev(p))
                assert np.array_equal(_u64(out), exp), (fn.__name__, towers, p.shape)
                assert np.array_equal(_u64(A), a)  # out of place: the input is untouched
                _check_lib(ck, out, towers, ch.L)
                assert _canonical(_u64(out), q)
                inplace = A.clone()
                assert fn(ck, inplace, _dev(p), out=inplace) is inplace
                assert np.array_equal(_u64(inplace), exp), (fn.__name__, towers, p.shape, "in place")
                if fn is not D.mult_plain:
                    assert np.array_equal(_u64(out)[:, 1], a[:, 1])  # c1 bit-identical
        exp = P.sub(a, b, q)
        out = D.sub(ck, A, B)
        assert np.array_equal(_u64(out), exp) and _canonical(exp, q)
        _check_lib(ck, out, towers, ch.L)
        for alias in (0, 1):  # out = a, out = b
            ins = [A.clone(), B.clone()]
            assert D.sub(ck, ins[0], ins[1], out=ins[alias]) is ins[alias]
            assert np.array_equal(_u64(ins[alias]), exp)
        assert not _u64(D.sub(ck, A, A)).any()
        n1 = D.neg(ck, A)
        assert np.array_equal(_u64(n1), P.neg(a, q)) and _canonical(_u64(n1), q)
        _check_lib(ck, n1, towers, ch.L)
        assert np.array_equal(_u64(D.neg(ck, n1)), a)
        assert D.neg(ck, n1, out=n1) is n1 and np.array_equal(_u64(n1), a)


# ------------------------------------------------------------- 5. values ----
# (batch, multDepth, ringDim): 2^13 / L3 and the sparse context (batch 4096 on ring 2^15)
VALUE_CASES = {"n13_L3": (4096, 2, 8192), "n15_sparse": (4096, 3, 32768)}


@functools.lru_cache(maxsize=None)
def keyed(cid):
    batch, depth, rd = VALUE_CASES[cid]
    ck = m.CKKS("ckks", batch, 52, "", multDepth=depth, ringDim=rd, seed=77, decodeNoise=False)
    assert ck.genCryptoContextAndKeyGen() == 1
    inf = ck.info()
    assert inf["ring_dim"] == rd
    return ck, inf


@pytest.mark.parametrize("cid", list(VALUE_CASES))
def test_values(cid):
    ck, inf = keyed(cid)
    S, L, d, q = inf["batch"], inf["num_towers"], inf["delta"], inf["moduli"]
    tol = max(1e-7, 2.0 ** (18 - 52))
    rng = np.random.default_rng(L)
    n = 2 * S
    x, y, z = (rng.uniform(-1, 1, n) for _ in range(3))
    cx, cz = D.encrypt(ck, _x(x)), D.encrypt(ck, _x(z))
    prod = D.rescale(ck, D.mult_plain(ck, cx, D.encode(ck, _x(y), towers=L, scale=float(q[L - 1]))))
    assert prod.shape[2] == L - 1
    assert np.abs(D.decrypt(ck, prod, n, d).cpu().numpy() - x * y).max() < tol
    py = D.encode(ck, _x(y))
    assert np.abs(D.decrypt(ck, D.add_plain(ck, cx, py), n, d).cpu().numpy() - (x + y)).max() < tol
    assert np.abs(D.decrypt(ck, D.sub_plain(ck, cx, py), n, d).cpu().numpy() - (x - y)).max() < tol
    assert np.abs(D.decrypt(ck, D.sub(ck, cx, cz), n, d).cpu().numpy() - (x - z)).max() < tol
    assert np.abs(D.decrypt(ck, D.neg(ck, cx), n, d).cpu().numpy() + x).max() < tol
    # one mask for every ciphertext
    mask = (np.arange(S) % 3 == 0).astype(np.float64)
    pm = D.encode(ck, _x(mask), towers=L, scale=float(q[L - 1]))
    got = D.decrypt(ck, D.rescale(ck, D.mult_plain(ck, cx, pm)), n, d).cpu().numpy()
    assert np.abs(got - x * np.tile(mask, 2)).max() < tol


# ------------------------------------------------------------ 6. no keys ----
def test_no_keys_needed():
    """A context that never had keys against a keyed one of the same parameters, bit for bit."""
    ck, inf = keyed("n13_L3")
    bk = m.CKKS("ckks", 4096, 52, "", multDepth=2, ringDim=8192, seed=1, decodeNoise=False)
    assert not bk.info()["keys_loaded"] and bk.info()["moduli"] == inf["moduli"]
    S, L = inf["batch"], inf["num_towers"]
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, 2 * S + 9)
    pts = [_encode(c, x) for c in (ck, bk)]
    assert np.array_equal(pts[0], pts[1])
    ct = D.encrypt(ck, _x(rng.uniform(-1, 1, 3 * S)))
    ct2 = D.encrypt(ck, _x(rng.uniform(-1, 1, 3 * S)))
    pt = _dev(pts[0])
    for fn in (D.mult_plain, D.add_plain, D.sub_plain):
        assert torch.equal(fn(ck, ct, pt), fn(bk, ct, pt))
    assert torch.equal(D.sub(ck, ct, ct2), D.sub(bk, ct, ct2))
    assert torch.equal(D.neg(ck, ct), D.neg(bk, ct))


# -------------------------------------------------------- 7. composition ----
def test_distance_with_one_hot_extraction():
    """||u - v||^2 = eval_sum((u - v)^2), then slot 0 picked out by a one-hot plaintext.  Levels and
    scales on the L = 3 chain: d = u - v (3 towers, delta); d d rescaled (2 towers, delta^2 / q_2);
    EvalSum (the same); times e_0 encoded over 2 towers at scale q_1 and rescaled (1 tower,
    delta^2 / q_2).  The last level is one 60-bit tower at a 52-bit scale: it holds values below 2^7,
    so u, v are sized for a sum of about 7 ("The sum must fit the level it sits on")."""
    ck, inf = keyed("n13_L3")
    ck.evalMultKeyGen()
    ck.evalSumKeyGen()
    S, d, q = inf["batch"], inf["delta"], inf["moduli"]
    tol = max(1e-7, 2.0 ** (18 - 52))
    rng = np.random.default_rng(7)
    K = 2
    u, v = rng.uniform(-0.05, 0.05, K * S), rng.uniform(-0.05, 0.05, K * S)
    diff = D.sub(ck, D.encrypt(ck, _x(u)), D.encrypt(ck, _x(v)))
    sq = D.rescale(ck, D.mult(ck, diff, diff))
    tot = D.eval_sum(ck, sq, S)
    e0 = np.zeros(S)
    e0[0] = 1.0
    pick = D.rescale(ck, D.mult_plain(ck, tot, D.encode(ck, _x(e0), towers=2, scale=float(q[1]))))
    assert tuple(pick.shape) == (K, 2, 1, inf["ring_dim"])
    got = D.decrypt(ck, pick, K * S, d * d / q[2]).cpu().numpy().reshape(K, S)
    exp = ((u - v) ** 2).reshape(K, S).sum(axis=1)
    assert 1.0 < exp.min() and exp.max() < 2.0 ** 6
    assert np.abs(got[:, 0] - exp).max() < math.sqrt(S) * tol
    assert np.abs(got[:, 1:]).max() < tol


# ------------------------------------------------------------- 8. guards ----
def test_guards():
    ck, inf = keyed("n13_L3")
    S, L, N = inf["batch"], inf["num_towers"], inf["ring_dim"]
    ck.evalMultKeyGen()
    a = D.encrypt(ck, _x(np.random.default_rng(8).uniform(-1, 1, 3 * S)))
    D.rescale(ck, D.mult(ck, a, a))
    chains = ck.eval_chunk_count()
    assert chains >= 1
    x = _x(np.ones(S + 1))
    sentinel = 0x5A5A5A5A5A5A5A5A

    def refused(call, out):
        out.fill_(sentinel)
        with pytest.raises(ValueError):
            call(out)
        torch.cuda.synchronize()
        assert bool((out == sentinel).all())
        assert ck.eval_chunk_count() == chains

    lib = _lib.load()

    def raw_encode(towers, scale):
        def call(out):
            _lib.check(lib.shelfi_dev_encode(ck._ctx, C.c_void_p(x.data_ptr()), x.numel(), towers, scale,
                                             C.c_void_p(out.data_ptr()), None))
        return call

    pt_out = torch.empty((2, L + 1, N), dtype=torch.int64, device="cuda")
    for towers in (0, L + 1):
        refused(raw_encode(towers, inf["delta"]), pt_out)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        refused(raw_encode(L, scale), pt_out)
        refused(lambda out, s=scale: D.encode(ck, x, scale=s, out=out), torch.empty((2, L, N), dtype=torch.int64,
                                                                                  device="cuda"))
    with pytest.raises(ValueError):
        D.encode(ck, x, towers=0)
    with pytest.raises(ValueError):
        D.encode(ck, x, towers=L + 1)
    with pytest.raises(ValueError):
        D.encode(ck, x.float())
    with pytest.raises(ValueError):
        D.encode(ck, x, out=torch.empty((2, L, N + 1), dtype=torch.int64, device="cuda"))

    pt3 = D.encode(ck, _x(np.ones(3 * S)))
    out = torch.empty_like(a)
    raw = {"mult": lib.shelfi_dev_mult_plain, "add": lib.shelfi_dev_add_plain, "sub": lib.shelfi_dev_sub_plain}
    for fn in raw.values():
        for K, Kp, towers in ((3, 2, L), (3, 3, 0), (3, 3, L + 1)):
            refused(lambda o, fn=fn, K=K, Kp=Kp, towers=towers: _lib.check(
                fn(ck._ctx, C.c_void_p(a.data_ptr()), C.c_void_p(pt3.data_ptr()), K, Kp, towers,
                   C.c_void_p(o.data_ptr()), None)), out)
        assert fn(ck._ctx, None, None, 0, 1, L, None, None) == 0  # K = 0: a successful no-op
        assert fn(ck._ctx, None, C.c_void_p(pt3.data_ptr()), 3, 3, L, C.c_void_p(out.data_ptr()), None) == _lib.SHELFI_ERR_ARG
    for towers in (0, L + 1):
        refused(lambda o, t=towers: _lib.check(lib.shelfi_dev_sub(ck._ctx, C.c_void_p(a.data_ptr()),
                                                                  C.c_void_p(a.data_ptr()), 3, t,
                                                                  C.c_void_p(o.data_ptr()), None)), out)
        refused(lambda o, t=towers: _lib.check(lib.shelfi_dev_negate(ck._ctx, C.c_void_p(a.data_ptr()), 3, t,
                                                                     C.c_void_p(o.data_ptr()), None)), out)
    assert lib.shelfi_dev_sub(ck._ctx, None, None, 0, L, None, None) == 0
    assert lib.shelfi_dev_negate(ck._ctx, None, 0, L, None, None) == 0
    assert lib.shelfi_dev_encode(ck._ctx, None, 0, L, inf["delta"], None, None) == 0
    # the Python layer's shape checks
    for fn in (D.mult_plain, D.add_plain, D.sub_plain):
        for bad in (pt3[:2], pt3[:, :2], pt3[:, :, :N // 2].contiguous(), pt3.cpu(), pt3.int()):
            refused(lambda o, fn=fn, bad=bad: fn(ck, a, bad, out=o), out)
        with pytest.raises(ValueError):
            fn(ck, a, pt3, out=out[:2])
    for bad in (a[:2], a[:, :, :2].contiguous()):
        refused(lambda o, bad=bad: D.sub(ck, a, bad, out=o), out)
    with pytest.raises(ValueError):
        D.neg(ck, a, out=out[:2])
