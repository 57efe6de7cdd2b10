"""The smudging noise of the threshold partial decryption against the oracle's restatement of its stream
(oracle.threshold_noise; DESIGN.md §2.10 "Noise stream"), on test_gpu_threshold.py's parties and helpers.

The noise integers are taken out of a noisy partial as (noisy partial - sigma = 0 partial) through the
inverse NTT, per tower, and must be the same integers in every tower; the sigma = 0 partial itself is
pinned against Python-integer c0 + c1 s_i (test_gpu_threshold.py test 2, and per level below).

Tolerance.  The product evaluates Box-Muller in binary32 (box_muller, dev_common.h), the oracle in binary64,
so the integers are close, not equal: |e_gpu - e_ref| <= 1 + sigma 2^-10 on every coefficient.  That is a
condition, not a measurement: about 2^10 below sigma (a misplaced coefficient differs by about sigma
sqrt(2), so no layout error survives it) and 4x the most the binary32 rounding of u1 alone can cause (u1
within 2^-24 of 1 moves r by at most 2^-12).  At sigma = 3.19 the bound allows a difference of 1, at
rounding ties; the share of differing coefficients is capped at 2^-9 of a call's K N (the worst case of
that quantisation error landing on a half-integer).  Every comparison prints its measured
max |e_gpu - e_ref| / sigma (DESIGN.md §2.10 lists them).

Rings: test_gpu_threshold.py's SHAPES plus 2^12, 2^14 (R = 2, 8 rows: a column's block partly used) and
2^16 (R = 32, two blocks per column on 2^11 blocks).  Also here: the counter (g advances by K on every
call, sigma = 0 calls included; set_seed restarts it; the bytes API draws the same stream), every level
l <= L (truncated fresh ciphertexts and real ModReduce outputs), and planted extreme residues
(c0 = c1 = s = q - 1) through pd_store_pair's epilogue."""
import numpy as np
import pytest

import oracle as O
import test_gpu_threshold as TT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

RINGS = [(1024, 1, 52, 60, 4096), (1024, 1, 52, 60, 16384), (1024, 1, 52, 60, 65536)]
SHAPES = TT.SHAPES + RINGS
SIGMAS = [2.0 ** 20, 3.19]
SEED = 4242

_u64, _dev, _addmod, _submod, _mulmod = TT._u64, TT._dev, TT._addmod, TT._submod, TT._mulmod


@pytest.fixture(scope="module", params=SHAPES, ids=TT._id)
def T(request):
    return TT._setup(request.param)


@pytest.fixture(scope="module")
def T15():
    return TT._setup(TT.CFG3)


def noise_ints(noisy, plain, q, psi):
    """noisy - plain = NTT(e) per tower -> e [K][N], checked to be the same integers in every tower."""
    d = _submod(noisy, plain, q)
    out = []
    for k in range(d.shape[0]):
        es = [O.to_signed(O.ntt_inv(d[k, t], q[t], psi[t]), q[t]) for t in range(len(q))]
        for e in es[1:]:
            assert np.array_equal(e, es[0])
        out.append(es[0])
    return np.stack(out)


def check_stream(e, seed, g0, sigma, what):
    """e [K][N] against the oracle's ciphertexts g0 .. g0 + K - 1; returns max |e - ref| / sigma."""
    K, N = e.shape
    ref = np.stack([O.threshold_noise(seed, g0 + k, N, O.threshold_block_log(N.bit_length() - 1), sigma)
                    for k in range(K)])
    d = np.abs(e - ref)
    dev = float(d.max()) / sigma
    differ = int(np.count_nonzero(d))
    print("noise deviation %s sigma %g g %d..%d: max|e_gpu - e_ref| / sigma = %.3g (2^%.1f), %d of %d differ"
          % (what, sigma, g0, g0 + K - 1, dev, np.log2(dev) if dev else -np.inf, differ, d.size))
    assert d.max() <= 1 + sigma * 2.0 ** -10, (what, sigma, int(d.max()))
    if sigma < 512:  # the bound is a difference of at most 1: rounding ties only
        assert differ <= d.size * 2.0 ** -9, (what, sigma, differ)
    return dev


def noisy_pair(c, ct, sigma, seed=None):
    """(lead, main) noisy partials [K][l][N] as uint64 arrays; seed: set_seed first (g restarts at 0)."""
    if seed is not None:
        c.set_seed(seed)
    c.set_threshold_noise(sigma)
    try:
        return _u64(D.partial_decrypt(c, ct, True)), _u64(D.partial_decrypt(c, ct, False))
    finally:
        c.set_threshold_noise(0.0)


# ---------------------------------------------------------------------------- B
@pytest.mark.parametrize("sigma", SIGMAS, ids=["s2p20", "s3.19"])
def test_noise_matches_oracle_stream(T, sigma):
    i, c, q, psi, K = 1, T["cs"][1], T["q"], T["psi"], 2
    plain = [_u64(D.partial_decrypt(c, T["ct"], lead)) for lead in (True, False)]
    if T["shape"] in RINGS:  # the rings test_gpu_threshold.py does not visit: sigma = 0 against the host
        assert np.array_equal(plain[1], T["prod"][i])
        assert np.array_equal(plain[0], _addmod(T["res"][:, 0], T["prod"][i], q))
    try:
        lead, main = noisy_pair(c, T["ct"], sigma, SEED)
    finally:
        c.set_seed(TT.SEEDS[i])
    what = "N=2^%d L=%d q0~2^%d" % (T["N"].bit_length() - 1, T["L"], int(q[0]).bit_length())
    check_stream(noise_ints(lead, plain[0], q, psi), SEED, 0, sigma, what + " lead")
    check_stream(noise_ints(main, plain[1], q, psi), SEED, K, sigma, what + " main")


@pytest.mark.parametrize("shape", [TT.CFG3, TT.SHAPES[4], RINGS[2]], ids=TT._id)
def test_counter_advances_on_every_call_and_bytes_api_draws_the_same_stream(shape):
    T = TT._setup(shape)
    q, psi, sigma = T["q"], T["psi"], 2.0 ** 20
    f = TT._new(shape, 77)
    f.set_keys(T["pk_joint"], T["sks"][1])
    ct3 = torch.cat([T["ct"], T["ct"][:1]]).contiguous()
    f.set_threshold_noise(0.0)
    plain3 = _u64(D.partial_decrypt(f, ct3, True))  # not yet seeded with SEED: only the arithmetic
    f.set_seed(SEED)
    assert np.array_equal(_u64(D.partial_decrypt(f, T["ct"], True)), plain3[:2])  # sigma = 0, K = 2: g 0, 1
    f.set_threshold_noise(sigma)
    n3 = _u64(D.partial_decrypt(f, ct3, True))  # K = 3: g 2, 3, 4
    check_stream(noise_ints(n3, plain3, q, psi), SEED, 2, sigma, "counter after a sigma = 0 call")
    f.set_seed(SEED)
    a0 = _u64(D.partial_decrypt(f, T["ct"], True))  # g 0, 1 again
    a1 = _u64(D.partial_decrypt(f, T["ct"], False))  # g 2, 3
    check_stream(noise_ints(a0, plain3[:2], q, psi), SEED, 0, sigma, "counter after set_seed")
    assert np.array_equal(noise_ints(a1, _submod(plain3[:2], T["res"][:, 0], q), q, psi)[0],
                          noise_ints(n3, plain3, q, psi)[0])  # g = 2 both times: the same integers
    # the bytes API on a same-seeded context: the same payloads at the same g
    b = TT._new(shape, SEED)
    b.set_keys(T["pk_joint"], T["sks"][1])
    blob = T["cs"][0].encrypt(T["x"])
    ctb = _dev(np.array(m.blob_residues(blob, T["N"], T["L"])))
    f.set_seed(SEED)
    for lead in (True, False):  # g 0, 1 then 2, 3 on both contexts
        pay = np.frombuffer(b.partialDecrypt(blob, lead), np.uint64, offset=64).reshape(2, T["L"], T["N"])
        assert np.array_equal(pay, _u64(D.partial_decrypt(f, ctb, lead)))


# ---------------------------------------------------------------------------- E
def _levels(T):
    """Level-l ciphertexts [2][2][l][N] with their scale: the first l towers of the fresh ciphertexts (a
    valid level-l ciphertext of the same plaintext), and real ModReduce outputs of the weight-1 aggregate
    (scale delta^2) at l = 4, 3, 2."""
    if "levels" not in T:
        c0, ct, q, delta = T["cs"][0], T["ct"], T["q"], T["delta"]
        lv = {("trunc", l): (ct[:, :, :l, :].contiguous(), delta) for l in range(1, T["L"] + 1)}
        a4 = D.wavg(c0, [ct], [1.0])
        a3 = D.rescale(c0, a4)
        a2 = D.rescale(c0, a3)
        s4 = delta * delta
        s3 = s4 / float(q[3])
        lv[("rescale", 4)], lv[("rescale", 3)], lv[("rescale", 2)] = (a4, s4), (a3, s3), (a2, s3 / float(q[2]))
        T["levels"] = lv
    return T["levels"]


@pytest.mark.parametrize("kind,l", [("trunc", 1), ("trunc", 2), ("trunc", 3), ("trunc", 4), ("rescale", 4),
                                    ("rescale", 3), ("rescale", 2)])
def test_levels_below_L(T15, kind, l):
    T = T15
    ct, scale = _levels(T)[(kind, l)]
    assert tuple(ct.shape) == (2, 2, l, T["N"])
    q, psi, S, n = T["q"][:l], T["psi"][:l], T["S"], T["n"]
    res = _u64(ct)
    ps, tot = [], None
    for i, c in enumerate(T["cs"]):
        pr = _mulmod(res[:, 1], T["sks"][i][:l], q)
        main, lead = D.partial_decrypt(c, ct, False), D.partial_decrypt(c, ct, True)
        assert np.array_equal(_u64(main), pr)
        assert np.array_equal(_u64(lead), _addmod(res[:, 0], pr, q))
        ps.append(lead if i == 0 else main)
        tot = _u64(ps[-1]) if tot is None else _addmod(tot, _u64(ps[-1]), q)
        if i == 1:
            for sigma in SIGMAS:
                try:
                    nl, nm = noisy_pair(c, ct, sigma, SEED)
                finally:
                    c.set_seed(TT.SEEDS[i])
                check_stream(noise_ints(nl, _u64(lead), q, psi), SEED, 0, sigma, "%s l=%d lead" % (kind, l))
                check_stream(noise_ints(nm, _u64(main), q, psi), SEED, 2, sigma, "%s l=%d main" % (kind, l))
    srv = TT._new(T["shape"], 96)
    fused = D.fuse_decrypt(srv, ps, n, scale).cpu().numpy()
    single = D.decrypt(T["cs"][0], _dev(TT._as_ct(tot)), n, scale).cpu().numpy()
    assert np.array_equal(fused.view(np.uint64), single.view(np.uint64))
    ref = O.decrypt_vector(res, T["sk_sum"][:l], q, psi, S, scale, n)
    assert np.array_equal(fused, ref)
    if kind == "trunc" or l >= 3:  # rescale l = 2 sits at scale ~1: nothing of x is left to compare
        assert np.abs(fused - T["x"]).max() < 1e-7


# ---------------------------------------------------------------------------- F
EXTREME_SHAPES = [TT.SHAPES[4], TT.SHAPES[0], TT.SHAPES[3], TT.SHAPES[5]]  # 2^11, 2^13, 2^17, 30-bit primes


@pytest.mark.parametrize("shape", EXTREME_SHAPES, ids=TT._id)
def test_partial_decrypt_planted_extremes(shape):
    """sk = q_t - 1 everywhere is NTT of the constant -1 (set_keys checks range, not pairing).  With
    c0 = c1 = q_t - 1: c1 s = (-1)(-1) = 1, so at sigma = 0 main is 1 and lead is 0 everywhere, and under
    noise lead is exactly NTT(e).  With c1 = 0 and c0 uniform: main is NTT(e), lead c0 + NTT(e)."""
    T = TT._setup(shape)
    q, psi, L, N, K, sigma = T["q"], T["psi"], T["L"], T["N"], 2, 2.0 ** 20
    top = np.broadcast_to((q - np.uint64(1))[:, None], (L, N))
    f = TT._new(shape, SEED)
    f.set_keys(T["pk_joint"], np.ascontiguousarray(top))
    ct = np.ascontiguousarray(np.broadcast_to(top, (K, 2, L, N)))
    ctd = _dev(ct)
    zero = np.zeros((K, L, N), np.uint64)
    f.set_threshold_noise(0.0)
    assert np.array_equal(_u64(D.partial_decrypt(f, ctd, True)), zero)
    assert np.array_equal(_u64(D.partial_decrypt(f, ctd, False)), zero + np.uint64(1))
    what = "extremes N=2^%d q0~2^%d" % (N.bit_length() - 1, int(q[0]).bit_length())
    lead, main = noisy_pair(f, ctd, sigma, SEED)
    check_stream(noise_ints(lead, zero, q, psi), SEED, 0, sigma, what + " lead")
    check_stream(noise_ints(main, zero + np.uint64(1), q, psi), SEED, K, sigma, what + " main")
    # c1 = 0, c0 uniform below q_t
    rng = np.random.default_rng(N)
    ct2 = np.zeros((K, 2, L, N), np.uint64)
    for t in range(L):
        ct2[:, 0, t] = rng.integers(0, int(q[t]), (K, N), dtype=np.uint64)
    ct2[0, 0, :, :3] = top[:, :3]  # and the largest residue in a few places
    ctd2 = _dev(ct2)
    assert np.array_equal(_u64(D.partial_decrypt(f, ctd2, True)), ct2[:, 0])
    assert np.array_equal(_u64(D.partial_decrypt(f, ctd2, False)), zero)
    lead, main = noisy_pair(f, ctd2, sigma, SEED)
    check_stream(noise_ints(lead, ct2[:, 0], q, psi), SEED, 0, sigma, what + " c1=0 lead")
    check_stream(noise_ints(main, zero, q, psi), SEED, K, sigma, what + " c1=0 main")
