"""The flooded half of launch_decrypt (PALISADE's decode noise, on by default) against the oracle on every
branch of its dispatch tree, every slot count and planted statistics (tests/flood_cases.py).

Branches: decode_flood_kernel below 2^6 slots (S = 1, 2, 32); decode_stats_kernel (G = S/2048 workgroups) with
the noise added by the single pass fft_fwd_blocks<true> (S = 64 .. 1024) or by fft_fwd_cols<LOGR, true>
(LOGR = 1 .. 5; LOGR = 5 at 2^16 slots draws two ChaCha blocks per thread); fft_fwd_whole<true> with
fft_whole_flood_stats and flood_add_kernel from 128 ciphertexts at 2^14 slots; the generic fft_fwd_blocks<false>
under SHELFI_FFT_CT=0; the chunk loops of dev_api.cpp and bytes_api.cpp (g0 and the flag reset per chunk).

Tolerance.  The product evaluates Box-Muller in binary32 (box_muller, dev_common.h), the oracle in binary64.
For every slot of every compared ciphertext

    |fl_gpu - fl_ref| <= 1e-14 max(1, max|fl_ref|) + 2^-10 B

with B = nsd_ref sqrt(S) from 64 slots on (output-domain noise, one normal per slot) and nsd_ref 2S below
(input-domain noise: a slot is a sum of 2S normals with unit-modulus coefficients), nsd_ref = sd_ref / 2^p
from the oracle.  The first term is test_gpu_decode_noise.py's own tolerance; the exact decode under it is
bit-equal to the oracle.  The second is the condition test_gpu_threshold_stream.py states for the same
function: each normal within 2^-10 of the oracle's, 4x what the binary32 rounding of u1 alone can cause and
about 2^10 below a misplaced normal.  At m_factor = 2^40 - 1 the second term dominates, and a relative error
eps in sigma, in sqrt(M + 1) or in 2^p moves an output by up to about 4 eps B: any eps above about 2^-12
fails.  Every comparison prints its measured max|fl_gpu - fl_ref| / B (DESIGN.md lists the largest per
shape).  No slot is left out.  Every compared call also asserts the failure verdict, last_log_precision() ==
p - max logError_ref, and that the flooded output is not the exact one.

set_seed() precedes every flooded call unless a test says otherwise, so the call's ciphertext k draws stream
index g = k."""
import math
import os

import numpy as np
import pytest

import flood_cases as F
import oracle as O
from conftest import set_switch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

M_BIG = F.M_BIG
SEED = 9001
TOO_HIGH = "approximation error is too high"
# (the same tuples as the sweep's rows, so each shape has one context and one key set in the module)
C13 = (4096, 8192, 1, 52, 60)    # 2^13 / L2: fft_fwd_cols<2, true>, G = 2
C14 = (8192, 16384, 2, 52, 60)   # 2^14 / L3: <3, true>, G = 4
C15 = (16384, 32768, 3, 52, 60)  # 2^15 / L4: <4, true>, G = 8; fft_fwd_whole<true> from K = 128


# ------------------------------------------------------------------ contexts ----
_made = {}


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    """ctx(shape) -> (CKKS, Shape); shape = (batch, ringDim, multDepth, scaleBits, firstModBits).  One context
    per shape for the module, keys from genCryptoContextAndKeyGen under a fixed seed."""
    def get(shape):
        if shape not in _made:
            batch, ring, depth, sb, fb = shape
            d = str(tmp_path_factory.mktemp("keys_flood")) + os.sep
            ck = m.CKKS("ckks", batch, sb, d, multDepth=depth, firstModBits=fb, ringDim=ring,
                        seed=100 + len(_made), decodeNoise=False)
            assert ck.genCryptoContextAndKeyGen() == 1
            inf = ck.info()
            assert inf["batch"] == batch and (not ring or inf["ring_dim"] == ring)
            _made[shape] = (ck, F.Shape.of(inf))
        return _made[shape]
    yield get
    _made.clear()


def _dev(res):
    return torch.from_numpy(np.ascontiguousarray(res).view(np.int64)).cuda()


def _exact(ck, sh, api, cts, n):
    if api == "bytes":
        return np.asarray(ck.decrypt(cts if isinstance(cts, bytes) else m.blob_pack(ck, cts), n))
    ct = cts if torch.is_tensor(cts) else _dev(cts)
    return D.decrypt(ck, ct, n, sh.delta).cpu().numpy()


def _flooded(ck, sh, api, cts, n, M=M_BIG, seed=SEED):
    """One flooded decrypt of residues / a blob / a device tensor -> (values, last_log_precision).  seed None:
    the counter goes on from where it is."""
    if seed is not None:
        ck.set_seed(seed)
    ck.set_decode_noise(True, M)
    try:
        out = _exact(ck, sh, api, cts, n)
        return out, ck.last_log_precision()
    finally:
        ck.set_decode_noise(False)


# ---------------------------------------------------------------- comparison ----
def _real(sh, res, sk, n, g, M, seed=SEED):
    """The oracle's verdict on a real ciphertext's residues [2][T][N] under the secret key."""
    T = res.shape[1]
    q, psi, sk = sh.q[:T], sh.psi[:T], np.ascontiguousarray(sk[:T])
    re, im = O.decrypt_coeffs(res, sk, q, psi, sh.S, sh.delta)
    sd, le, fail = O.decode_stats(re, im, sh.N, sh.p_bits, M)
    v = F.Verdict("real", 1.0, res, sd, le, fail)
    v.fl, le2, fail2 = O.decrypt_flood(res, sk, q, psi, sh.S, sh.delta, n, seed=seed, g=g, p_bits=sh.p_bits,
                                       m_factor=M)
    assert (le2, fail2) == (le, fail)
    return v


def _compare(what, sh, fl, refs, n):
    """fl: the call's n values; refs: {ciphertext index: Verdict with .fl}.  Every slot of each listed
    ciphertext under the module's tolerance; returns the largest max|fl_gpu - fl_ref| / B."""
    worst, bad = 0.0, []
    for k, v in sorted(refs.items()):
        ln = min(sh.S, n - k * sh.S)
        assert ln > 0 and v.fl.shape == (ln,) and not v.fail
        got = fl[k * sh.S:k * sh.S + ln]
        B = v.bound(sh)
        d = float(np.abs(got - v.fl).max())
        tol = 1e-14 * max(1.0, float(np.abs(v.fl).max())) + 2.0 ** -10 * B
        worst = max(worst, d / B)
        print("flood ratio %s S=%d N=%d ct %d %s: max|fl_gpu - fl_ref| / B = %.3g (2^%.1f), B = %.3g"
              % (what, sh.S, sh.N, k, v.case, d / B, math.log2(d / B) if d else -math.inf, B))
        if not d <= tol:
            bad.append((k, v.case, d, tol, d / B))
    assert not bad, (what, bad)  # every ciphertext that misses, not only the first
    return worst


def _check_call(what, ck, sh, api, cts, n, refs, M=M_BIG, seed=SEED, all_le=None):
    """A flooded call against the oracle: the listed ciphertexts' slots, the precision (all_le: the logErrors
    of every ciphertext of the call when refs lists only some), and that noise was added."""
    exact = _exact(ck, sh, api, cts, n)
    fl, prec = _flooded(ck, sh, api, cts, n, M, seed)
    _compare("%s %s" % (what, api), sh, fl, refs, n)
    les = [v.le for v in refs.values()] if all_le is None else list(all_le)
    assert prec == sh.p_bits - max(les), (what, prec, les)
    for k in refs:  # every compared ciphertext carries noise
        seg = slice(k * sh.S, min(n, (k + 1) * sh.S))
        assert not np.array_equal(fl[seg], exact[seg]), (what, k)
    return fl


# ============================================================ A. dispatch sweep ====
ROWS = [  # (batch, ringDim, multDepth, scaleBits, firstModBits): the branch
    (1, 2048, 1, 52, 60),        # decode_flood_kernel, S == 1: sigma = |im_0|
    (2, 2048, 1, 52, 60),        # decode_flood_kernel, only i = 0 and i = half
    (32, 2048, 1, 52, 60),       # decode_flood_kernel
    (64, 2048, 1, 52, 60),       # first fused size: fft_fwd_blocks<true>, S16 = 4, G = 1 with 31 pairs
    (1024, 2048, 1, 52, 60),     # the largest single pass, gap 1
    (2048, 4096, 1, 52, 60),     # fft_fwd_cols<1, true>
    (4096, 8192, 1, 52, 60),     # <2, true>, G = 2
    (8192, 16384, 2, 52, 60),    # <3, true>, G = 4
    (16384, 32768, 3, 52, 60),   # <4, true>, K < 128
    (32768, 65536, 1, 52, 60),   # 2^11 FFT blocks, <4, true>
    (65536, 131072, 1, 52, 60),  # <5, true>: two ChaCha blocks per thread
    (4096, 0, 1, 30, 40),        # p_bits = 30
]
_rows = {}


def _row(ctx, shape):
    """A row's real encryptions (K = 3 of uniform(-1, 1) float32 values where the batch allows, the last one
    partial) and their exact decode, held to the oracle's bit for bit."""
    if shape not in _rows:
        ck, sh = ctx(shape)
        n = 2 * sh.S + sh.S // 3
        K = -(-n // sh.S)
        x = np.random.default_rng(sh.S).uniform(-1, 1, n).astype(np.float32).astype(np.float64)
        ck.set_seed(SEED)
        blob = ck.encrypt(x)
        res = np.array(m.blob_residues(blob, sh.N, len(sh.q)))
        assert res.shape[0] == K
        _, sk = ck.get_keys()
        exact = ck.decrypt(blob, n)
        assert np.array_equal(exact, O.decrypt_vector(res, sk, sh.q, sh.psi, sh.S, sh.delta, n))
        assert np.abs(exact - x).max() < max(1e-7, 2.0 ** (18 - sh.p_bits))
        _rows[shape] = (blob, res, sk, n, K)
    return _rows[shape]


@pytest.mark.parametrize("M", [1.0, M_BIG], ids=["M1", "Mbig"])
@pytest.mark.parametrize("shape", ROWS, ids=lambda s: "b%d_n%d_d%d_s%d" % s[:4])
def test_dispatch_sweep_against_oracle(ctx, shape, M):
    ck, sh = ctx(shape)
    blob, res, sk, n, K = _row(ctx, shape)
    refs = {k: _real(sh, res[k], sk, min(sh.S, n - k * sh.S), k, M) for k in range(K)}
    _check_call("sweep M=%g" % M, ck, sh, "bytes", blob, n, refs, M)
    _check_call("sweep M=%g" % M, ck, sh, "device", res, n, refs, M)


@pytest.mark.parametrize("shape", [ROWS[5], ROWS[9]], ids=["b2048", "b32768"])
def test_generic_block_pass_then_flooded_columns(ctx, shape, monkeypatch):
    """SHELFI_FFT_CT=0: fft_fwd_blocks<false> (the LDS-loop block pass) followed by fft_fwd_cols<LOGR, true>."""
    ck, sh = ctx(shape)
    blob, res, sk, n, K = _row(ctx, shape)
    ref, prec = _flooded(ck, sh, "device", res, n)
    set_switch(monkeypatch, "SHELFI_FFT_CT", "0")
    got, prec0 = _flooded(ck, sh, "device", res, n)
    assert np.array_equal(got, ref) and prec0 == prec


def test_whole_vector_path_against_oracle(ctx, monkeypatch):
    """129 ciphertexts at 2^14 slots: fft_fwd_whole<true> + flood_add_kernel, the last ciphertext partial (rem)."""
    ck, sh = ctx(C15)
    K, n = 129, 128 * sh.S + 5
    g = torch.Generator(device="cuda").manual_seed(129)
    x = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    ck.set_seed(SEED + 1)
    ct = D.encrypt(ck, x)
    assert ct.shape[0] == K
    _, sk = ck.get_keys()
    fl, prec = _flooded(ck, sh, "device", ct, n)
    res = ct.cpu().numpy().view(np.uint64)
    refs = {k: _real(sh, res[k], sk, min(sh.S, n - k * sh.S), k, M_BIG) for k in (0, 1, 127, 128)}
    _compare("whole", sh, fl, refs, n)
    les = [O.decode_stats(*O.decrypt_coeffs(res[k], sk, sh.q, sh.psi, sh.S, sh.delta), sh.N, sh.p_bits, M_BIG)[1]
           for k in range(K)]
    assert prec == sh.p_bits - max(les)
    assert not np.array_equal(fl, _exact(ck, sh, "device", ct, n))
    set_switch(monkeypatch, "SHELFI_FFT_WHOLE", "0")
    got, prec0 = _flooded(ck, sh, "device", ct, n)
    assert np.array_equal(got, fl) and prec0 == prec


# ======================================================= B. planted statistics ====
STATS = {  # the four implementations of the statistics
    "decode_flood_kernel": (32, 2048, 1, 52, 60),
    "decode_stats_kernel G=1": (64, 2048, 1, 52, 60),
    "decode_stats_kernel G=4": C14,
}
_planted = {}


def _cases(sh, key, ids, M=M_BIG, g0=0):
    """Verdicts of the cases `ids` as ciphertexts g0, g0 + 1, ... of one call (shared by the tests of a shape)."""
    out = []
    for k, case in enumerate(ids):
        kk = (key, case, M, g0 + k)
        if kk not in _planted:
            _planted[kk] = F.build(sh, case, M, seed=SEED, g=g0 + k)
        out.append(_planted[kk])
    return out


def _stack(vs):
    return np.stack([v.res for v in vs])


@pytest.mark.parametrize("api", ["bytes", "device"])
@pytest.mark.parametrize("impl", list(STATS))
def test_planted_statistics(ctx, impl, api):
    """Every planted case but P5b as one ciphertext of one call (case k draws stream index k)."""
    ck, sh = ctx(STATS[impl])
    ids = [c for c in F.case_ids(sh.S) if c != "P5b"]
    vs = _cases(sh, impl, ids)
    _check_call(impl, ck, sh, api, _stack(vs), len(vs) * sh.S, dict(enumerate(vs)))


@pytest.mark.parametrize("api", ["bytes", "device"])
@pytest.mark.parametrize("impl", list(STATS))
def test_planted_case_alone_decides_the_calls_log_error(ctx, impl, api):
    """In the call above the largest logError (P5a's) hides every other one behind atomicMax.  Here every case
    is a call of its own (K = 1, stream index 0), so the device's logError of that case -- the floor's formula
    for P0, P0z, P2b, P3x and P4c, and the 32-slot shape's rint at a half-integer -- is what
    last_log_precision() reports."""
    ck, sh = ctx(STATS[impl])
    assert ROWS.count(STATS[impl]) == 1
    for case in F.case_ids(sh.S):
        if case == "P5b":
            continue
        v = _cases(sh, impl + " alone", [case])[0]
        fl, prec = _flooded(ck, sh, api, v.res[None], sh.S)
        assert prec == sh.p_bits - v.le, (impl, case, prec, v.le)
        _compare("%s alone %s" % (impl, api), sh, fl, {0: v}, sh.S)
        assert not np.array_equal(fl, v.exact), case


ALONE_WHOLE = ["P0", "P0z", "P2b", "P3x@1", "P4c", "P1", "P2a", "P3@1", "P4", "P6"]


def test_whole_vector_one_case_per_call(ctx):
    """fft_whole_flood_stats with the case under test deciding the call's logError: 128 copies of one case per
    call (the first and the last ciphertext against the oracle at their own stream indices)."""
    ck, sh = ctx(C15)
    for case in ALONE_WHOLE:
        v = F.build(sh, case, M_BIG)
        ct = _dev(v.res).unsqueeze(0).expand(128, -1, -1, -1).contiguous()
        fl, prec = _flooded(ck, sh, "device", ct, 128 * sh.S)
        assert prec == sh.p_bits - v.le, (case, prec, v.le)
        _compare("fft_whole_flood_stats %s x 128" % case, sh, fl, {k: _at(sh, v, k) for k in (0, 127)}, 128 * sh.S)


@pytest.mark.parametrize("impl", list(STATS))
def test_planted_precision_failure_raises_and_the_context_recovers(ctx, impl):
    ck, sh = ctx(STATS[impl])
    bad, good = _cases(sh, impl, ["P6", "P5b", "P6"]), _cases(sh, impl, ["P6"])
    assert [v.fail for v in bad] == [False, True, False]
    for api in ("bytes", "device"):
        with pytest.raises(RuntimeError, match=TOO_HIGH):
            _flooded(ck, sh, api, _stack(bad), 3 * sh.S)
        _check_call(impl + " after P5b", ck, sh, api, _stack(good), sh.S, {0: good[0]})
    # without flooding nothing is estimated and nothing raises
    assert np.array_equal(_exact(ck, sh, "device", _stack(bad), 3 * sh.S)[sh.S:2 * sh.S], bad[1].exact)


def test_planted_statistics_whole_vector(ctx):
    """fft_whole_flood_stats: the case list tiled over the 128 ciphertexts of one call, each with its own stream
    index; then P5b among 127 others in a call of its own."""
    ck, sh = ctx(C15)
    ids = [c for c in F.case_ids(sh.S) if c != "P5b"]
    base = {c: F.build(sh, c, M_BIG) for c in ids}
    tiled = [ids[k % len(ids)] for k in range(128)]
    res = np.stack([base[c].res for c in tiled])
    nokey = np.zeros((len(sh.q), sh.N), np.uint64)
    refs = {}
    for k, c in enumerate(tiled):
        b = base[c]
        v = F.Verdict(c, b.amp, b.res, b.sd, b.le, b.fail)
        v.fl, le, fail = O.decrypt_flood(b.res, nokey, sh.q, sh.psi, sh.S, sh.delta, sh.S, seed=SEED, g=k,
                                         p_bits=sh.p_bits, m_factor=M_BIG)
        assert (le, fail) == (b.le, b.fail)
        refs[k] = v
    ct = _dev(res)
    _check_call("fft_whole_flood_stats", ck, sh, "device", ct, 128 * sh.S, refs)
    bad = F.build(sh, "P5b", M_BIG)
    assert bad.fail
    ct[77] = _dev(bad.res)
    with pytest.raises(RuntimeError, match=TOO_HIGH):
        _flooded(ck, sh, "device", ct, 128 * sh.S)
    ct[77] = _dev(base["P6"].res)
    fl, _ = _flooded(ck, sh, "device", ct, 128 * sh.S)
    refs = {k: refs[k] for k in (0, 76, 78, 127)}
    _compare("fft_whole_flood_stats after P5b", sh, fl, refs, 128 * sh.S)


@pytest.mark.parametrize("M", [0.0, 1.0, 3.0], ids=["M0", "M1", "M3"])
def test_m_factor(ctx, M):
    """sqrt(M + 1) at small M (P6: estimated sigma_p ~ 3000, far above the floor)."""
    ck, sh = ctx(C13)
    vs = _cases(sh, "c13", ["P6"], M)
    for api in ("bytes", "device"):
        _check_call("P6 M=%g" % M, ck, sh, api, _stack(vs), sh.S, {0: vs[0]}, M)


# ========================================================== C. seams, variants ====
def _ladder(sh, key, K, descending=False, slot=1):
    """K built ciphertexts whose sigma differs: P3 with A, 2A, 4A, ... (the largest first if descending); their
    flooded references are made per call (the stream index is the position)."""
    amps = [2.0 ** j for j in range(K)]
    if descending:
        amps.reverse()
    out = []
    for a in amps:
        kk = (key, a, slot)
        if kk not in _planted:
            _planted[kk] = F.build(sh, "P3@%d" % slot, M_BIG, amp=a)
        out.append(_planted[kk])
    return out


def _at(sh, v, g, M=M_BIG, seed=SEED, n=None):
    """Verdict v's flooded reference at stream index g."""
    T = v.res.shape[1]
    n = sh.S if n is None else n
    w = F.Verdict(v.case, v.amp, v.res, v.sd, v.le, v.fail)
    w.fl, le, fail = O.decrypt_flood(v.res, np.zeros((T, sh.N), np.uint64), sh.q[:T], sh.psi[:T], sh.S, sh.delta, n,
                                     seed=seed, g=g, p_bits=sh.p_bits, m_factor=M)
    assert (le, fail) == (v.le, v.fail)
    return w


def _decode_towers(sh):
    bits = 0
    for t, q in enumerate(sh.q):
        bits += int(q).bit_length() - 1
        if bits > 130:
            return t + 1
    return len(sh.q)


def _dev_chunks(sh, K, mib):
    """dev_api.cpp's dev_chunk() over decrypt_scratch_bytes(): the chunk sizes of a K-ciphertext device decrypt
    under SHELFI_DEV_CHUNK_MIB = mib."""
    G = max(1, sh.S // 2 // 1024)
    per = _decode_towers(sh) * sh.N * 8 + sh.S * 16 + G * 16 + 64
    cap = max(1, (mib << 20) // per)
    nch = -(-K // cap)
    kc = -(-K // nch)
    return [min(kc, K - k0) for k0 in range(0, K, kc)]


@pytest.mark.parametrize("shape,K,mib,chunks", [(C13, 11, 1, [4, 4, 3]), (C15, 5, 3, [2, 2, 1])],
                         ids=["2^13_K11", "2^15_K5"])
def test_device_chunks(ctx, monkeypatch, shape, K, mib, chunks):
    """SHELFI_DEV_CHUNK_MIB with noise on: chunk c's ciphertexts draw g0 + k0 + k, the logError is the maximum over
    the chunks (the flags are reset by the first chunk only), a failure in a later chunk still raises.  The
    switch counts whole MiB, so at 2^13 / L2 (192 KiB of scratch per ciphertext) the smallest budget holds 5
    ciphertexts: K = 11 splits 4, 4, 3 there, and K = 5 splits 2, 2, 1 at 2^15 / L4 under 3 MiB."""
    ck, sh = ctx(shape)
    assert _dev_chunks(sh, K, mib) == chunks and _dev_chunks(sh, K, 4096) == [K]
    for descending in (False, True):
        vs = _ladder(sh, shape, K, descending)
        les = [v.le for v in vs]
        assert len(set(les)) == K and les.index(max(les)) == (0 if descending else K - 1)
        res = _stack(vs)
        whole, prec = _flooded(ck, sh, "device", res, K * sh.S)
        set_switch(monkeypatch, "SHELFI_DEV_CHUNK_MIB", str(mib))
        refs = {k: _at(sh, v, k) for k, v in enumerate(vs)}
        fl = _check_call("chunks %s" % chunks, ck, sh, "device", res, K * sh.S, refs)
        assert np.array_equal(fl, whole)
        assert prec == sh.p_bits - max(les)
        # a failing ciphertext in the second chunk
        bad = res.copy()
        k_bad = chunks[0] + 1
        bad[k_bad] = F.build(sh, "P5b", M_BIG).res
        with pytest.raises(RuntimeError, match=TOO_HIGH):
            _flooded(ck, sh, "device", bad, K * sh.S)
        set_switch(monkeypatch, "SHELFI_DEV_CHUNK_MIB", None)


def test_bytes_decrypt_chunks(ctx):
    """The bytes decrypt uploads 64 MiB chunks of the decode's tower prefix: 3 towers, 1.5 MiB per ciphertext at
    2^15 / L4, so 42 ciphertexts per chunk and ciphertext 42 of 43 alone in the second (dn.g0 += kc, no reset)."""
    ck, sh = ctx(C15)
    assert _decode_towers(sh) == 3 and (64 << 20) // (2 * 3 * sh.N * 8) == 42
    K, n = 43, 43 * sh.S
    four = _ladder(sh, C15, 4)
    top = F.build(sh, "P3@1", M_BIG, amp=2.0 ** 6)  # decides the logError, at index 42
    vs = [four[k % 4] for k in range(42)] + [top]
    assert top.le > max(v.le for v in four)
    res = _stack(vs)
    refs = {k: _at(sh, vs[k], k) for k in (0, 41, 42)}
    fl = _check_call("bytes chunks", ck, sh, "bytes", m.blob_pack(ck, res), n, refs, all_le=[v.le for v in vs])
    dev, prec = _flooded(ck, sh, "device", res, n)
    assert np.array_equal(fl, dev) and prec == sh.p_bits - top.le
    # a failure in the second chunk
    bad = res.copy()
    bad[42] = F.build(sh, "P5b", M_BIG).res
    with pytest.raises(RuntimeError, match=TOO_HIGH):
        _flooded(ck, sh, "bytes", m.blob_pack(ck, bad), n)


def test_bytes_decrypt_chunks_packed_blob(ctx):
    """The same seam through a packed blob (unpacked on the device per chunk).  No entry point packs chosen
    residues, so these are real encryptions: ciphertexts 0, 41 and 42 against the oracle, the whole output
    against the device decrypt of the unpacked residues."""
    ck, sh = ctx(C15)
    K, n = 43, 43 * sh.S - 7
    x = np.random.default_rng(43).uniform(-1, 1, n)
    ck.set_seed(SEED + 2)
    ck.set_wire_format("packed")
    try:
        blob = ck.encrypt(x)
    finally:
        ck.set_wire_format("palisade")
    assert m.blob_info(blob)["format"] == "packed" and m.blob_info(blob)["num_cts"] == K
    res = m.blob_residues(blob, sh.N, len(sh.q), ckks=ck)
    _, sk = ck.get_keys()
    refs = {k: _real(sh, res[k], sk, min(sh.S, n - k * sh.S), k, M_BIG) for k in (0, 41, 42)}
    fl, prec = _flooded(ck, sh, "bytes", blob, n)
    _compare("packed bytes chunks", sh, fl, refs, n)
    dev, prec_dev = _flooded(ck, sh, "device", res, n)
    assert np.array_equal(fl, dev) and prec == prec_dev
    assert not np.array_equal(fl, _exact(ck, sh, "bytes", blob, n))


def test_noise_counter(ctx):
    """A flooded decrypt of K ciphertexts advances the context's stream by K, as an encrypt does; set_seed
    restarts it; the device API and the bytes API draw the same indices from the same state."""
    ck, sh = ctx(C13)
    vs = _ladder(sh, C13, 3)
    res, n = _stack(vs), 3 * sh.S
    a, _ = _flooded(ck, sh, "device", res, n)            # g 0..2
    b, _ = _flooded(ck, sh, "device", res, n, seed=None)  # g 3..5
    _compare("counter first call", sh, a, {k: _at(sh, v, k) for k, v in enumerate(vs)}, n)
    _compare("counter second call", sh, b, {k: _at(sh, v, 3 + k) for k, v in enumerate(vs)}, n)
    a2, _ = _flooded(ck, sh, "bytes", res, n)             # set_seed: 0..2 again, through the bytes API
    assert np.array_equal(a2, a)
    ck.encrypt(np.zeros(2 * sh.S))                        # two ciphertexts: g 3, 4
    c, _ = _flooded(ck, sh, "bytes", res, n, seed=None)   # g 5..7
    _compare("counter after an encrypt", sh, c, {k: _at(sh, v, 5 + k) for k, v in enumerate(vs)}, n)
    ck.set_seed(SEED)
    D.encrypt(ck, torch.zeros(2 * sh.S, dtype=torch.float64, device="cuda"))
    d, _ = _flooded(ck, sh, "device", res, n, seed=None)  # g 2..4
    _compare("counter after a device encrypt", sh, d, {k: _at(sh, v, 2 + k) for k, v in enumerate(vs)}, n)


@pytest.mark.parametrize("l", [1, 2, 3, 4])
def test_levels(ctx, l):
    """Built ciphertexts of l towers at scale delta through device.decrypt, against the oracle over q[:l]."""
    ck, sh = ctx(C15)
    shl = F.Shape.of(ck.info(), towers=l)
    vs = [F.build(shl, c, M_BIG, seed=SEED, g=k) for k, c in enumerate(["P6", "P3@1", "P4"])]
    res = _stack(vs)
    assert res.shape == (3, 2, l, sh.N)
    _check_call("level l=%d" % l, ck, shl, "device", res, 3 * sh.S, dict(enumerate(vs)))
    for case in ("P0", "P3@1", "P4"):  # and alone, so that each one's logError is the call's
        v = F.build(shl, case, M_BIG, seed=SEED, g=0)
        _check_call("level l=%d alone" % l, ck, shl, "device", v.res[None], sh.S, {0: v})


@pytest.mark.parametrize("K", [3, 96], ids=["oneshot", "persistent"])
def test_decrypt_sum_flooded(ctx, K):
    """Residues x + k q (k <= 15) through decrypt_sum's folding first pass, flooded: bit-equal to the flooded
    decrypt of x at the same seed (K = 96: 96 x 3 x 16 >= 4096 items, the persistent pass)."""
    ck, sh = ctx(C15)
    four = _ladder(sh, C15, 4)
    h = _stack([four[k % 4] for k in range(K)])
    n = K * sh.S - 3
    k = np.random.default_rng(K).integers(0, 16, h.shape, dtype=np.uint64)
    k[0, 0, 0, :8] = 15
    lazy = h + k * sh.q[None, None, :, None]
    ref, prec = _flooded(ck, sh, "device", h, n)
    if K == 3:
        _compare("decrypt_sum reference", sh, ref, {j: _at(sh, four[j], j, n=min(sh.S, n - j * sh.S))
                                                    for j in range(3)}, n)
    ck.set_seed(SEED)
    ck.set_decode_noise(True, M_BIG)
    try:
        got = D.decrypt_sum(ck, _dev(lazy), 16, n, sh.delta).cpu().numpy()
        assert ck.last_log_precision() == prec
    finally:
        ck.set_decode_noise(False)
    assert np.array_equal(got, ref)
    assert not np.array_equal(got, _exact(ck, sh, "device", h, n))


def test_fusion_flooded():
    """Flooded fuse_decrypt of sigma = 0 partials == the flooded decrypt of the same ciphertexts under the joint
    key at the same seed (test_gpu_threshold.py's parties), on its smallest shape and on 2^15 / L4."""
    import test_gpu_threshold as TT

    for shape in (TT.SHAPES[4], TT.CFG3):
        T = TT._setup(shape)
        ps = [D.partial_decrypt(c, T["ct"], i == 0) for i, c in enumerate(T["cs"])]
        srv, joint = TT._new(shape, 91), TT._new(shape, 92)
        joint.set_keys(T["pk_joint"], T["sk_sum"])
        outs = []
        for c, call in ((srv, lambda: D.fuse_decrypt(srv, ps, T["n"], T["delta"])),
                        (joint, lambda: D.decrypt(joint, T["ct"], T["n"], T["delta"]))):
            exact = call().cpu().numpy()
            c.set_seed(SEED)
            c.set_decode_noise(True, M_BIG)
            try:
                outs.append((call().cpu().numpy(), c.last_log_precision(), exact))
            finally:
                c.set_decode_noise(False)
        (f, pf, ef), (j, pj, ej) = outs
        assert np.array_equal(ef, ej) and np.array_equal(f, j) and pf == pj
        assert not np.array_equal(f, ef)
        sh = F.Shape.of(T["cs"][0].info())
        refs = {k: _real(sh, T["res"][k], T["sk_sum"], min(sh.S, T["n"] - k * sh.S), k, M_BIG) for k in range(2)}
        _compare("fusion", sh, f, refs, T["n"])
        assert pf == sh.p_bits - max(v.le for v in refs.values())


SWITCHES = [("SHELFI_XCD_ORDER", "0"), ("SHELFI_NTT_WL", "0"), ("SHELFI_DEC_PP", "0"),
            ("SHELFI_DEC_ALL_TOWERS", "1"), ("SHELFI_FFT_CT", "0")]
_sw = {}


@pytest.mark.parametrize("var,val", SWITCHES, ids=lambda v: str(v))
def test_decrypt_switches_under_flooding(ctx, monkeypatch, var, val):
    ck, sh = ctx(C15)
    if "ref" not in _sw:
        g = torch.Generator(device="cuda").manual_seed(7)
        n = 7 * sh.S - 3
        x = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
        ck.set_seed(SEED + 3)
        ct = D.encrypt(ck, x)
        fl, prec = _flooded(ck, sh, "device", ct, n)
        _, sk = ck.get_keys()
        _compare("switches reference", sh, fl, {6: _real(sh, ct[6].cpu().numpy().view(np.uint64), sk, sh.S - 3, 6,
                                                         M_BIG)}, n)
        _sw["ref"] = (ct, n, fl, prec)
    ct, n, fl, prec = _sw["ref"]
    set_switch(monkeypatch, var, val)
    got, prec0 = _flooded(ck, sh, "device", ct, n)
    assert np.array_equal(got, fl) and prec0 == prec, var
