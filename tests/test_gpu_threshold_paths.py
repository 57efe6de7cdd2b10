"""Every path the threshold calls can take, against the paths already pinned (test_gpu_threshold.py's
parties and helpers).

C. The persistent fusion pass (ntt_inv_blocks_dec_pp<.., FuseIn>, from 4,096 (ciphertext, tower, block)
   items) at every branch of its prefetch: P = 1 (partial 1 never read), 2 (nothing summed in the prefetch),
   3 (the odd tail alone), 4 (one pair), 15 (six pairs and the tail), 16 (seven pairs); both wave-local
   templates (SHELFI_NTT_WL) and the one-shot pass at the same K (SHELFI_DEC_PP=0); over the 3-tower prefix
   (K = 96: 4,608 items) and over every tower (SHELFI_DEC_ALL_TOWERS=1, K = 70: 4,480 items).
D. The A/B switches that reach the fused and the noisy kernels, and SHELFI_DEV_CHUNK_MIB on the partial
   decryption (input, output, scratch and the noise counter offset per chunk), the fusion (every partial's
   pointer offset per chunk) and the flooded fusion: bit-identical to the default path, and the chunked
   noise still the oracle's ciphertexts g0 + k0 + k.
F. Planted extreme residues through the fused loaders: 16 partials of q_t - 1 sum to 16 (q_t - 1), the
   largest word the SUM reduction can meet.

Fusions are compared bit for bit with device.decrypt of the host-summed (sum of partials mod q, 0) and with
the oracle's decrypt of that ciphertext (c1 = 0: the key does not enter)."""
import numpy as np
import pytest

import oracle as O
import test_gpu_threshold as TT
from conftest import set_switch
from test_gpu_threshold_stream import SEED, check_stream, noise_ints

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from SHELFI_FHE import device as D  # noqa: E402

_u64, _dev = TT._u64, TT._dev


@pytest.fixture(scope="module")
def T15():
    return TT._setup(TT.CFG3)


def _qs(T, l=None):
    return torch.tensor(T["q"][:l].astype(np.int64), device="cuda").view(1, -1, 1)


def _fold(parts, qs):
    """Sum of canonical partials mod q_t on the device (two residues below 2^60: the int64 sum is exact)."""
    tot = parts[0]
    for p in parts[1:]:
        s = tot + p
        tot = torch.where(s >= qs, s - qs, s)
    return tot


def _as_ct(tot):
    ct = torch.zeros((tot.shape[0], 2) + tuple(tot.shape[1:]), dtype=torch.int64, device=tot.device)
    ct[:, 0] = tot
    return ct


def _batch(T, K, seed):
    """K ciphertexts of an n that ends inside the last one, and the three parties' sigma = 0 partials."""
    n = K * T["S"] - 5
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    x = x * 2 - 1
    ct = D.encrypt(T["cs"][0], x)
    ps = [D.partial_decrypt(c, ct, i == 0) for i, c in enumerate(T["cs"])]
    return dict(K=K, n=n, x=x, ct=ct, ps=ps)


# ---------------------------------------------------------------------------- C
PS = [1, 2, 3, 4, 15, 16]


@pytest.fixture(scope="module")
def big(T15):
    """K = 96 at 2^15 / L4 (K = 70: its first 70 ciphertexts), and per (K, P) the reference: device.decrypt of
    the host-folded sum on the default path, its first ciphertext checked against the oracle."""
    T = T15
    B = _batch(T, 96, 96)
    qs, S, delta = _qs(T), T["S"], T["delta"]
    refs = {}
    for K in (96, 70):
        n = K * S - 5
        for P in PS:
            parts = [p[:K] for p in (B["ps"] * 6)[:P]]
            tot = _fold(parts, qs)
            single = D.decrypt(T["cs"][0], _as_ct(tot), n, delta)
            if K == 96:
                ref = O.decrypt_vector(_u64(_as_ct(tot[:1])), T["sk_sum"], T["q"], T["psi"], S, delta, S)
                assert np.array_equal(single[:S].cpu().numpy(), ref), P
            refs[(K, P)] = single
    assert float((refs[(96, 3)] - B["x"]).abs().max()) < 1e-7  # P = 3: the whole key, the plaintext itself
    B["refs"] = refs
    B["srv"] = TT._new(T["shape"], 98)  # a server context that never had keys
    return B


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("K,towers", [(96, "prefix"), (70, "all")])
@pytest.mark.parametrize("path", ["pp_wl", "pp_nowl", "oneshot"])
def test_fusion_large_batch_every_P(T15, big, monkeypatch, path, K, towers, P):
    T = T15
    if towers == "all":
        set_switch(monkeypatch, "SHELFI_DEC_ALL_TOWERS", "1")
    if path == "pp_nowl":
        set_switch(monkeypatch, "SHELFI_NTT_WL", "0")
    if path == "oneshot":
        set_switch(monkeypatch, "SHELFI_DEC_PP", "0")
    n = K * T["S"] - 5
    parts = [p[:K] for p in (big["ps"] * 6)[:P]]
    fused = D.fuse_decrypt(big["srv"], parts, n, T["delta"])
    assert torch.equal(fused.view(torch.int64), big["refs"][(K, P)].view(torch.int64))


# ---------------------------------------------------------------------------- D
SWITCHES = [("SHELFI_DEC_PP", "0"), ("SHELFI_XCD_ORDER", "0"), ("SHELFI_NTT_WL", "0"), ("SHELFI_FFT_CT", "0"),
            ("SHELFI_FFT_WHOLE", "0"), ("SHELFI_DEC_ALL_TOWERS", "1")]


def _threshold_calls(T, B, srv, srvn):
    """The calls under test at one counter position: a sigma = 0 call first (g0 = K for what follows), then
    the seeded noisy lead and main partials of party 1, the fusion of the three sigma = 0 partials, and the
    flooded fusion on a seeded context."""
    c, sigma = T["cs"][1], 2.0 ** 20
    c.set_seed(SEED)
    try:
        c.set_threshold_noise(0.0)
        plain = D.partial_decrypt(c, B["ct"], False)
        c.set_threshold_noise(sigma)
        lead, main = D.partial_decrypt(c, B["ct"], True), D.partial_decrypt(c, B["ct"], False)
    finally:
        c.set_threshold_noise(0.0)
        c.set_seed(TT.SEEDS[1])
    fused = D.fuse_decrypt(srv, B["ps"], B["n"], T["delta"])
    srvn.set_seed(SEED)
    flooded = D.fuse_decrypt(srvn, B["ps"], B["n"], T["delta"])
    return dict(plain=plain, lead=lead, main=main, fused=fused, flooded=flooded)


def _same(a, b, tag):
    for k in a:
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), (tag, k)


@pytest.fixture(scope="module")
def small(T15):
    T = T15
    out = {}
    for K in (7, 5):
        B = _batch(T, K, K)
        B["srv"], B["srvn"] = TT._new(T["shape"], 95), TT._new(T["shape"], 94, noise=True)
        B["ref"] = r = _threshold_calls(T, B, B["srv"], B["srvn"])
        # the default path itself: the fusion against the single-key decrypt and the plaintext, the flooded
        # fusion close to it, the noise the oracle's ciphertexts K .. 3K - 1 (after the sigma = 0 call)
        tot = _fold(B["ps"], _qs(T))
        single = D.decrypt(T["cs"][0], _as_ct(tot), B["n"], T["delta"])
        assert torch.equal(r["fused"].view(torch.int64), single.view(torch.int64))
        assert float((r["fused"] - B["x"]).abs().max()) < 1e-7
        assert not torch.equal(r["flooded"], r["fused"]) and float((r["flooded"] - B["x"]).abs().max()) < 1e-6
        _check_noise(T, B, r)
        out[K] = B
    return out


def _check_noise(T, B, r):
    q, psi, K, sigma = T["q"], T["psi"], B["K"], 2.0 ** 20
    plain = _u64(r["plain"])
    assert np.array_equal(plain, _u64(B["ps"][1]))
    c0 = _u64(B["ct"])[:, 0]
    check_stream(noise_ints(TT._submod(_u64(r["lead"]), c0, q), plain, q, psi), SEED, K, sigma, "K=%d lead" % K)
    check_stream(noise_ints(_u64(r["main"]), plain, q, psi), SEED, 2 * K, sigma, "K=%d main" % K)


@pytest.mark.parametrize("var,val", SWITCHES, ids=lambda v: str(v))
def test_threshold_switch_bitexact(T15, small, monkeypatch, var, val):
    B = small[7]
    set_switch(monkeypatch, var, val)
    _same(_threshold_calls(T15, B, B["srv"], B["srvn"]), B["ref"], var)


@pytest.mark.parametrize("mib", ["2", "1"])
def test_threshold_chunked_calls_bitexact(T15, small, monkeypatch, mib):
    """K = 5 at 2^15 / L4: the noisy partial's scratch is 1 MiB per ciphertext, so "2" gives chunks 2, 2, 1
    and "1" one chunk per ciphertext; the fusion splits by decrypt's own scratch per ciphertext (the prefix's
    towers and the FFT buffer), several chunks under either value.  Chunk c's ciphertexts carry
    g = g0 + k0 + k: the chunked noise is compared with the oracle's stream again, not only with the
    unchunked call."""
    B = small[5]
    set_switch(monkeypatch, "SHELFI_DEV_CHUNK_MIB", mib)
    got = _threshold_calls(T15, B, B["srv"], B["srvn"])
    _same(got, B["ref"], "chunk " + mib)
    _check_noise(T15, B, got)


# ---------------------------------------------------------------------------- F
EXTREME_SHAPES = [TT.SHAPES[4], TT.SHAPES[0], TT.SHAPES[3], TT.SHAPES[5]]  # 2^11, 2^13, 2^17, 30-bit primes


@pytest.mark.parametrize("shape", EXTREME_SHAPES, ids=TT._id)
def test_fusion_planted_extremes(shape):
    """Every residue q_t - 1 is the evaluation form of the constant polynomial -1, whose decode is -1 / scale
    in every slot.  Scale 16: 16 partials of q_t - 1 (the summed word 16 (q_t - 1), the largest the loaders
    can see) decode to -1.0; 16 partials alternating 0 and q_t - 1, by partial and by element (each element
    sums 8 (q_t - 1)), to -0.5; one partial of q_t - 1 to -0.0625."""
    T = TT._setup(shape)
    q, psi, L, N, S, n, K, scale = T["q"], T["psi"], T["L"], T["N"], T["S"], T["n"], 2, 16.0
    top = np.ascontiguousarray(np.broadcast_to((q - np.uint64(1))[:, None], (K, L, N)))
    even = top.copy()
    even[..., 1::2] = 0
    odd = top.copy()
    odd[..., 0::2] = 0
    dtop, deven, dodd = _dev(top), _dev(even), _dev(odd)
    srv = TT._new(shape, 93)
    qs = _qs(T)
    for parts, want in (([dtop] * 16, -1.0), ([deven, dodd] * 8, -0.5), ([dtop], -0.0625)):
        fused = D.fuse_decrypt(srv, parts, n, scale)
        tot = _fold(parts, qs)
        single = D.decrypt(T["cs"][0], _as_ct(tot), n, scale)
        assert torch.equal(fused.view(torch.int64), single.view(torch.int64)), want
        ref = O.decrypt_vector(_u64(_as_ct(tot)), T["sk_sum"], q, psi, S, scale, n)
        out = fused.cpu().numpy()
        assert np.array_equal(out, ref), want
        assert np.abs(out - want).max() <= 1e-12, want
