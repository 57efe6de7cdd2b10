"""Threshold CKKS on the MI355X (the reference's code/mkhe/mkhe.cpp RunCKKS, lines 188-465): the key chain
(MultipartyKeyGen, :268-282), each party's partial decryption (MultipartyDecryptLead / Main, :395-400) and
the fusion (MultipartyDecryptFusion, :402).

Three parties (seeds 11, 12, 13) with identical parameters: party 0 generates keys, parties 1 and 2 chain
multipartyKeyGen, all install (pk_joint, own share).  The issue's four (batch, multDepth) cases give rings
2^13 (twice: ParamsGen's 128-bit ring for L = 2 is 2^13 at batch 1024 too), 2^15 / L4 (the prefix decode
with fused CRT columns) and 2^17 (2^12 blocks); two more cases reach what those leave out: ringDim = 2^11
(one NTT block: no columns pass, the noise sampled on load) and 30-bit scaling primes (q < 2^40: the
generic passes behind a columns pass).

Bit-exact where the arithmetic is deterministic: the chain against the oracle's keygen stream and NTT,
the sigma = 0 partials against c0 + c1 s_i on the host (Python integers), the fusion against the
single-key device decrypt of (sum of the partials, 0) and against the oracle's decrypt under sum s_i.
The smudging noise is checked here as what it must be -- one integer polynomial per ciphertext, the same in
every tower, of the set standard deviation, never repeated, reproducible under a seed; its stream is held
against the oracle's restatement (oracle.threshold_noise) in test_gpu_threshold_stream.py, and the paths
these K = 2 calls do not take (the persistent fusion pass at every P, switches, chunked calls, levels below
L, planted extremes) in test_gpu_threshold_paths.py.  PALISADE's own sampler stays unpinned.

Bounds: |mean| <= 5 sigma / sqrt(K N) (5 standard errors); the sample standard deviation within 5% of
sigma (its own spread at K N >= 4096 samples is below 1.2%; rounding adds 1/12 to the variance, 0.4% at
sigma = 3.19); max |e| <= 9 sigma (Box-Muller over 32-bit uniforms cannot pass 6.66 sigma).  End to end
the threshold result differs from the exact single-key decode D by the decode of sum e_i: at most
8 sigma sqrt(3 N) / Delta as the issue sets it (Delta = q_{L-1}; against the aggregate's scale Delta^2 the
noise itself is far smaller still, so the bound is met with a wide margin)."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

SEEDS = (11, 12, 13)
# (batch, multDepth, scaleBits, firstModBits, ringDim) with test_gpu_f4.py's CASES constructor arguments
SHAPES52 = [(1024, 1, 52, 60, 0), (4096, 1, 52, 60, 0), (16384, 3, 52, 60, 0), (65536, 1, 52, 60, 0),
            (1024, 1, 52, 60, 2048)]
SHAPES = SHAPES52 + [(4096, 1, 30, 40, 0)]
CFG3 = SHAPES[2]


def _new(shape, seed, noise=False):
    batch, depth, sb, fb, rd = shape
    return m.CKKS("ckks", batch, sb, "", multDepth=depth, firstModBits=fb, ringDim=rd, seed=seed,
                  decodeNoise=noise)


def _mulmod(a, b, q):
    """a * b mod q_t per tower, Python integers; a [..][L][N], b [L][N]."""
    out = np.empty(a.shape, np.uint64)
    for t, qt in enumerate(q):
        out[..., t, :] = ((a[..., t, :].astype(object) * b[t].astype(object)) % int(qt)).astype(np.uint64)
    return out


def _addmod(a, b, q):
    out = np.empty(a.shape, np.uint64)
    for t, qt in enumerate(q):
        qt = np.uint64(qt)
        s = a[..., t, :] + b[..., t, :]  # both below q_t < 2^60
        out[..., t, :] = np.where(s >= qt, s - qt, s)
    return out


def _submod(a, b, q):
    out = np.empty(a.shape, np.uint64)
    for t, qt in enumerate(q):
        qt = np.uint64(qt)
        out[..., t, :] = np.where(a[..., t, :] >= b[..., t, :], a[..., t, :] - b[..., t, :],
                                  a[..., t, :] + qt - b[..., t, :])
    return out


def _signed_mod(v, qt):
    return (v.astype(object) % int(qt)).astype(np.uint64)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@functools.lru_cache(maxsize=None)
def _setup(shape):
    batch, depth = shape[:2]
    cs = [_new(shape, s) for s in SEEDS]
    assert cs[0].genCryptoContextAndKeyGen() == 1
    keys = [cs[0].get_keys()]
    for i in (1, 2):
        cs[i].multipartyKeyGen(keys[-1][0])
        keys.append(cs[i].get_keys())
    pk_joint = keys[-1][0]
    for c, (_, sk) in zip(cs, keys):
        c.set_keys(pk_joint, sk)
        c.set_threshold_noise(0.0)
    inf = cs[0].info()
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    N, S, delta = inf["ring_dim"], inf["batch"], inf["delta"]
    sks = [k[1] for k in keys]
    sk_sum = sks[0]
    for s in sks[1:]:
        sk_sum = _addmod(sk_sum, s, q)
    # K = 2 ciphertexts of an n that ends inside the second one
    n = S + S // 2 + 3
    x = np.random.default_rng(batch + depth).uniform(-1, 1, n)
    tol = max(1e-7, 2.0 ** (18 - shape[2]))  # test_gpu_f4.py's value tolerance (noise ~ 2^-13 at 30-bit scale)
    ct = D.encrypt(cs[0], torch.from_numpy(x).cuda())
    res = _u64(ct)
    prod = [_mulmod(res[:, 1], s, q) for s in sks]  # c1 s_i  [K][L][N]
    return dict(cs=cs, keys=keys, pk_joint=pk_joint, sks=sks, sk_sum=sk_sum, q=q, psi=psi, N=N, S=S, L=len(q),
                delta=delta, n=n, x=x, ct=ct, res=res, prod=prod, shape=shape, tol=tol)


def _id(c):
    return "b%d_d%d_s%d%s" % (c[0], c[1], c[2], "_n%d" % c[4] if c[4] else "")


@pytest.fixture(scope="module", params=SHAPES, ids=_id)
def T(request):
    return _setup(request.param)


@pytest.fixture(scope="module", params=SHAPES52, ids=_id)
def T52(request):
    return _setup(request.param)


@pytest.fixture(scope="module")
def T15():
    return _setup(CFG3)


def _plain_partials(T):
    """The three sigma = 0 partials (party 0 the lead) on the device and their host sum."""
    ps = [D.partial_decrypt(c, T["ct"], i == 0) for i, c in enumerate(T["cs"])]
    tot = _addmod(_addmod(_u64(ps[0]), _u64(ps[1]), T["q"]), _u64(ps[2]), T["q"])
    return ps, tot


def _as_ct(c0):
    """(c0, c1 = 0) as a ciphertext batch [K][2][L][N]."""
    out = np.zeros((c0.shape[0], 2) + c0.shape[1:], np.uint64)
    out[:, 0] = c0
    return out


# ---------------------------------------------------------------------------- 1
def test_key_chain_bitexact(T):
    q, psi, N = T["q"], T["psi"], T["N"]
    for i in (1, 2):
        s, e, _ = O.sample_keygen(SEEDS[i], N, q)
        (pk, sk), prev = T["keys"][i], T["keys"][i - 1][0]
        ns = np.stack([O.ntt_fwd(_signed_mod(s, qt), qt, pt) for qt, pt in zip(q, psi)])
        ne = np.stack([O.ntt_fwd(_signed_mod(e, qt), qt, pt) for qt, pt in zip(q, psi)])
        assert np.array_equal(sk, ns)
        assert np.array_equal(pk[1], prev[1])
        assert np.array_equal(pk[0], _addmod(prev[0], _submod(ne, _mulmod(prev[1], sk, q), q), q))
    # b_joint + a sum s_i = sum e_i: small, and the same integers in every tower
    d = _addmod(T["pk_joint"][0], _mulmod(T["pk_joint"][1], T["sk_sum"], q), q)
    es = [O.to_signed(O.ntt_inv(d[t], q[t], psi[t]), q[t]) for t in range(T["L"])]
    for e in es[1:]:
        assert np.array_equal(e, es[0])
    assert np.abs(es[0]).max() <= 3 * (len(O.gauss_cdt()) - 1)
    assert np.abs(es[0]).max() > 0


# ---------------------------------------------------------------------------- 2
def test_partials_bitexact_without_noise(T):
    q, res = T["q"], T["res"]
    for i, c in enumerate(T["cs"]):
        main = _u64(D.partial_decrypt(c, T["ct"], False))
        lead = _u64(D.partial_decrypt(c, T["ct"], True))
        assert main.shape == (2, T["L"], T["N"])
        assert np.array_equal(main, T["prod"][i])
        assert np.array_equal(lead, _addmod(res[:, 0], T["prod"][i], q))
    if T["L"] >= 3:  # a ModReduce output: L - 1 towers
        c = T["cs"][1]
        r = D.rescale(c, T["ct"])
        rr = _u64(r)
        assert rr.shape[2] == T["L"] - 1
        ql = q[:T["L"] - 1]
        pr = _mulmod(rr[:, 1], T["sks"][1][:T["L"] - 1], ql)
        assert np.array_equal(_u64(D.partial_decrypt(c, r, False)), pr)
        assert np.array_equal(_u64(D.partial_decrypt(c, r, True)), _addmod(rr[:, 0], pr, ql))


# ---------------------------------------------------------------------------- 3
def test_fuse_bitexact_against_single_key_decrypt(T):
    q, psi, S, n, delta = T["q"], T["psi"], T["S"], T["n"], T["delta"]
    c0 = T["cs"][0]
    ps, tot = _plain_partials(T)
    fused = D.fuse_decrypt(c0, ps, n, delta).cpu().numpy()
    single = D.decrypt(c0, _dev(_as_ct(tot)), n, delta).cpu().numpy()
    assert np.array_equal(fused.view(np.uint64), single.view(np.uint64))
    ref = O.decrypt_vector(T["res"], T["sk_sum"], q, psi, S, delta, n)
    assert np.array_equal(fused, ref)
    assert np.abs(fused - T["x"]).max() < T["tol"]
    # a server context that never had keys
    srv = _new(T["shape"], 99)
    assert not srv.info()["keys_loaded"]
    assert np.array_equal(D.fuse_decrypt(srv, ps, n, delta).cpu().numpy(), fused)
    # P = 1 and P = 16 (the partials repeated; compared with the host sum's decrypt)
    one = D.fuse_decrypt(srv, ps[:1], n, delta).cpu().numpy()
    assert np.array_equal(one, D.decrypt(c0, _dev(_as_ct(_u64(ps[0]))), n, delta).cpu().numpy())
    many = (ps * 6)[:16]
    tot16 = _u64(many[0])
    for p in many[1:]:
        tot16 = _addmod(tot16, _u64(p), q)
    f16 = D.fuse_decrypt(srv, many, n, delta).cpu().numpy()
    assert np.array_equal(f16.view(np.uint64), D.decrypt(c0, _dev(_as_ct(tot16)), n, delta).cpu().numpy().view(np.uint64))


# ---------------------------------------------------------------------------- 4
def _noise_of(T, part, i, lead):
    """partial - ([c0 +] c1 s_i): the centred integers per ciphertext, checked equal across towers."""
    q, psi = T["q"], T["psi"]
    want = _addmod(T["res"][:, 0], T["prod"][i], q) if lead else T["prod"][i]
    d = _submod(part, want, q)
    out = []
    for k in range(d.shape[0]):
        es = [O.to_signed(O.ntt_inv(d[k, t], q[t], psi[t]), q[t]) for t in range(T["L"])]
        for e in es[1:]:
            assert np.array_equal(e, es[0])
        out.append(es[0])
    return np.stack(out)


@pytest.mark.parametrize("sigma", [2.0 ** 20, 3.19], ids=["s2p20", "s3.19"])
def test_noise_is_integer_sized_and_never_repeats(T, sigma):
    i, c = 1, T["cs"][1]
    c.set_threshold_noise(sigma)
    try:
        e1 = _noise_of(T, _u64(D.partial_decrypt(c, T["ct"], True)), i, True)
        e2 = _noise_of(T, _u64(D.partial_decrypt(c, T["ct"], False)), i, False)
    finally:
        c.set_threshold_noise(0.0)
    for e in (e1, e2):
        cnt = e.size
        assert cnt >= 4096
        print("sigma %g: mean %.4g std %.6g max %.4g over %d" % (sigma, e.mean(), e.std(), np.abs(e).max(), cnt))
        assert abs(e.mean()) <= 5 * sigma / np.sqrt(cnt)
        assert abs(e.std() / sigma - 1) <= 0.05
        assert np.abs(e).max() <= 9 * sigma
        assert not np.array_equal(e[0], e[1])  # the call's two ciphertexts
    assert not np.array_equal(e1, e2)  # a second call
    # two fresh contexts, same seed and call sequence: identical partials
    outs = []
    for _ in range(2):
        f = _new(T["shape"], 77)
        f.set_keys(T["pk_joint"], T["sks"][i])
        f.set_threshold_noise(sigma)
        outs.append((_u64(D.partial_decrypt(f, T["ct"], True)), _u64(D.partial_decrypt(f, T["ct"], False))))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert not np.array_equal(_noise_of(T, outs[0][0], i, True), e1)


# ---------------------------------------------------------------------------- 5
def test_end_to_end_bytes_api_with_default_noise(T52):
    """52-bit scale (a flooded decode of 2^20 smudging noise has no precision left at 30 bits)."""
    T = T52
    q, psi, N, S, delta, tol = T["q"], T["psi"], T["N"], T["S"], T["delta"], T["tol"]
    sigma = 2.0 ** 20
    n = S + 7
    rng = np.random.default_rng(5)
    xs = [rng.uniform(-1, 1, n) for _ in range(3)]
    w = [0.5, 0.3, 0.2]
    cs = [_new(T["shape"], 31 + i) for i in range(3)]  # fresh contexts: the default noise
    for c, sk in zip(cs, T["sks"]):
        c.set_keys(T["pk_joint"], sk)
    blobs = [c.encrypt(x) for c, x in zip(cs, xs)]
    agg = cs[0].computeWeightedAverage(blobs, w)
    parts = [c.partialDecrypt(agg, i == 0) for i, c in enumerate(cs)]
    for i, p in enumerate(parts):
        hi = m.partial_blob_info(p)
        assert hi["num_cts"] == 2 and hi["towers"] == T["L"] and hi["lead"] == (i == 0)
        assert hi["key_id"] == cs[0].info()["key_id"]
    srv = _new(T["shape"], 55)
    out = srv.fuseDecrypt(parts, n)
    bi = m.blob_info(agg)
    exact = O.decrypt_vector(m.blob_residues(agg, N, len(q)), T["sk_sum"], q, psi, S, bi["scale"], n)
    truth = sum(float(np.float32(wi)) * x for wi, x in zip(w, xs))
    bound = 8 * sigma * np.sqrt(3 * N) / delta
    print("threshold - single key: %.3g (bound %.3g); - truth: %.3g" %
          (np.abs(out - exact).max(), bound, np.abs(out - truth).max()))
    assert np.abs(out - exact).max() <= bound
    assert np.abs(out - truth).max() <= tol + bound
    # the partials do carry noise: the same call again gives other bytes
    assert cs[1].partialDecrypt(agg, False) != parts[1]
    # flooded decode (PALISADE's default) on the fusing side
    srvn = _new(T["shape"], 56, noise=True)
    outn = srvn.fuseDecrypt(parts, n)
    assert srvn.last_log_precision() is not None
    assert np.abs(outn - truth).max() < 1e-6


# ---------------------------------------------------------------------------- 6
def test_large_batch_dispatch(T15):
    """K = 128 at 2^15 / L4: the persistent first pass (K L' 16 >= 4096 items) and fft_fwd_whole."""
    T = T15
    c0, c1 = T["cs"][0], T["cs"][1]
    K, S, delta = 128, T["S"], T["delta"]
    n = K * S - 5
    x = torch.rand(n, dtype=torch.float64, device="cuda") * 2 - 1
    ct = D.encrypt(c0, x)
    ps = [D.partial_decrypt(c0, ct, True), D.partial_decrypt(c1, ct, False)]
    qs = torch.tensor(T["q"].astype(np.int64), device="cuda").view(1, -1, 1)
    tot = (ps[0] + ps[1]) % qs  # residues below 2^60: the int64 sum is exact
    eq = torch.zeros_like(ct)
    eq[:, 0] = tot
    srv = _new(T["shape"], 98)
    fused = D.fuse_decrypt(srv, ps, n, delta)
    single = D.decrypt(c0, eq, n, delta)
    assert torch.equal(fused.view(torch.int64), single.view(torch.int64))
    # the first ciphertext against the oracle (two of the three shares: not the plaintext)
    sk01 = _addmod(T["sks"][0], T["sks"][1], T["q"])
    ref = O.decrypt_vector(_u64(ct[:1]), sk01, T["q"], T["psi"], S, delta, S)
    assert np.array_equal(fused[:S].cpu().numpy(), ref)


# ---------------------------------------------------------------------------- 7
def test_wide_values_redo(T15):
    """test_gpu_decode_wide.py's 2^100 aggregate (|X| ~ 2^199: past the prefix's 2^127), split into two
    partials: the fusion is redone through the exact CRT exactly when the single-key decrypt is."""
    T = T15
    cs, q, S, delta = T["cs"], T["q"], T["S"], T["delta"]
    xm, w = 1e12 * 2.0 ** 60, [0.4, 0.3, 0.2, 0.1]
    rng = np.random.default_rng(100)
    sign = rng.choice([-1.0, 1.0], S)
    xs = [sign * rng.uniform(0.9, 1.0, S) * xm for _ in range(4)]
    exp = sum(float(np.float32(wi)) * x for wi, x in zip(w, xs))
    agg = D.wavg(cs[0], [D.encrypt(cs[0], torch.from_numpy(x).cuda()) for x in xs], w)
    p0 = D.partial_decrypt(cs[0], agg, True)
    rest = _addmod(_u64(D.partial_decrypt(cs[1], agg, False)), _u64(D.partial_decrypt(cs[2], agg, False)), q)
    ps = [p0, _dev(rest)]
    tot = _addmod(_u64(p0), rest, q)
    srv = _new(T["shape"], 97)
    scale = delta * delta
    r0 = cs[0].decode_redo_count()
    single = D.decrypt(cs[0], _dev(_as_ct(tot)), S, scale).cpu().numpy()
    assert cs[0].decode_redo_count() - r0 == 1  # |X| ~ 2^199: the single-key decrypt is redone
    s0 = srv.decode_redo_count()
    fused = D.fuse_decrypt(srv, ps, S, scale).cpu().numpy()
    assert srv.decode_redo_count() - s0 == 1
    assert np.array_equal(fused.view(np.uint64), single.view(np.uint64))
    assert np.abs(fused - exp).max() <= 2.0 ** -30 * np.abs(exp).max()  # test_gpu_decode_wide.py's bound
    # a narrow call on the same contexts: no redo on either side
    T_ps, T_tot = _plain_partials(T)
    r0, s0 = cs[0].decode_redo_count(), srv.decode_redo_count()
    a = D.decrypt(cs[0], _dev(_as_ct(T_tot)), T["n"], delta).cpu().numpy()
    b = D.fuse_decrypt(srv, T_ps, T["n"], delta).cpu().numpy()
    assert np.array_equal(a, b)
    assert cs[0].decode_redo_count() == r0 and srv.decode_redo_count() == s0


# ---------------------------------------------------------------------------- 8
def _code(exc):
    return exc.value.code


def test_guards(T15):
    T = T15
    c, L, S, delta = T["cs"][0], T["L"], T["S"], T["delta"]
    lib = _lib.load()
    ps, _ = _plain_partials(T)
    out = torch.empty(T["n"], dtype=torch.float64, device="cuda")
    stream = C.c_void_p(0)
    ptrs = (C.c_void_p * 17)(*([ps[0].data_ptr()] * 17))
    for P in (0, 17):
        assert lib.shelfi_dev_fuse_decrypt(c._ctx, ptrs, P, 2, L, delta, T["n"], C.c_void_p(out.data_ptr()),
                                           stream) == _lib.SHELFI_ERR_ARG
    for towers in (0, L + 1):
        assert lib.shelfi_dev_fuse_decrypt(c._ctx, ptrs, 3, 2, towers, delta, T["n"], C.c_void_p(out.data_ptr()),
                                           stream) == _lib.SHELFI_ERR_ARG
        assert lib.shelfi_dev_partial_decrypt(c._ctx, C.c_void_p(T["ct"].data_ptr()), 2, towers, 1,
                                              C.c_void_p(ps[0].data_ptr()), stream) == _lib.SHELFI_ERR_ARG
    with pytest.raises(ValueError):
        D.fuse_decrypt(c, ps, 2 * S + 1, delta)
    nokeys = _new(T["shape"], 3)
    with pytest.raises(m.ShelfiError) as ei:
        D.partial_decrypt(nokeys, T["ct"], True)
    assert _code(ei) == _lib.SHELFI_ERR_STATE
    with pytest.raises(m.ShelfiError) as ei:
        nokeys.partialDecrypt(c.encrypt(T["x"]), True)
    assert _code(ei) == _lib.SHELFI_ERR_STATE
    for bad in (-1.0, float("nan"), float("inf"), 2.0 ** 41):
        with pytest.raises(ValueError):
            c.set_threshold_noise(bad)
    c.set_threshold_noise(2.0 ** 40)
    c.set_threshold_noise(0.0)
    # the bytes fusion's header checks
    blob = c.encrypt(T["x"])
    lead, main = c.partialDecrypt(blob, True), T["cs"][1].partialDecrypt(blob, False)
    assert np.abs(c.fuseDecrypt([lead, main, T["cs"][2].partialDecrypt(blob, False)], T["n"]) - T["x"]).max() < 1e-7
    other_key = bytearray(main)
    other_key[48:56] = struct.pack("<Q", 12345)  # BlobHeader.key_id
    one_ct = main[:64 + (len(main) - 64) // 2]
    one_ct = one_ct[:16] + struct.pack("<Q", 1) + one_ct[24:]  # BlobHeader.K
    for bad in ([lead, lead], [main, main], [lead, bytes(other_key)], [lead, one_ct], [lead, main[:-8]],
                [lead, main[:40]]):
        with pytest.raises(m.ShelfiError) as ei:
            c.fuseDecrypt(bad, T["n"])
        assert _code(ei) == _lib.SHELFI_ERR_FORMAT
    pk = T["pk_joint"].copy()
    pk[0, 0, 5] = T["q"][0]
    with pytest.raises(m.ShelfiError) as ei:
        nokeys.multipartyKeyGen(pk)
    assert _code(ei) == _lib.SHELFI_ERR_FORMAT
    assert not nokeys.info()["keys_loaded"]
