"""Decrypt over the reference's whole value range (VERDICT r5 missing 1; ckks.cpp:189 cc->Decrypt ->
CRTInterpolate to a BigInteger, centred mod Q, then Decode, ckks.cpp:198-199).

The fast decode (crt_value over the shortest tower prefix above 2^130) is exact for centred values
|X| < 2^127 and flags every coefficient outside that range; the call is then redone over every
tower through crt_exact_kernel, exact up to (Q - 1) / 2 as PALISADE's BigInteger decode.  Every case
below is bit-exact vs the oracle's multi-word centring + Horner conversion (`or_crt_centered_double`)
and within the encoding's relative precision of the plaintext.

Which path a case takes is asserted, not assumed: `_coeff_range` takes the true largest decrypted
coefficient from the oracle (`O.decrypt_coeffs`) and every case states which side of 2^127 it lies on;
`CKKS.decode_redo_count()` is read around every decrypt call (1 more after a call with a wide
ciphertext, unchanged after a fast-path call and under set_decode_exact).  Slots of random sign put
only |x| Delta^d / sqrt(S)-sized values into the coefficients, far below the |x| Delta^d a one-signed
vector puts into the constant coefficient:

- fresh ciphertexts of |x| = 2^80 (|X| ~ 2^126: the fast path) and 2^120 (|X| ~ 2^166: redone) at
  2^15 / L4 and 2^16 / L6, through the device API and the bytes API;
- depth-2 aggregates of random-sign slots with |sum w x| ~ 2^23 (|X| ~ 2^121: the fast path), 2^60 and
  2^100 (|X| ~ 2^159, 2^199: redone), through both APIs;
- depth-2 aggregates of positive slots ~ 2^24 (the constant coefficient alone is past 2^127, by less
  than a bit) and 2^35, unflooded and flooded, through both APIs: the default mode after a real redo;
- a flooded decode of fresh 2^80 values fails on the fast path exactly where the oracle's Decode
  does, and one of fresh 2^120 values after the redo;
- a flooded 3-ciphertext call whose middle ciphertext alone is wide keeps every ciphertext's own
  noise stream through the redo.

Tolerances: bit-exact vs the oracle (noise-free decode); vs the plaintext 2^-36 relative for fresh
ciphertexts (the encode's logApprox scale-down keeps 62 bits), 2^-30 for aggregates (EvalMult's
W = (int64)(w Delta + 0.5) quantizes a weight w by 0.5 / (w Delta): 2^-34 relative at w = 2^-20).  The flooded decode compares with
the oracle within 1e-9 of the noise's own size (GPU vs glibc log/sincos of the same stream).
Parity with PALISADE itself is unpinned above 2^64 (BigInteger::ConvertToDouble's rounding)."""
import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402


def _make(tmp_path_factory, name, batch, depth, seed):
    d = str(tmp_path_factory.mktemp(name)) + os.sep
    ck = m.CKKS("ckks", batch, 52, d, multDepth=depth, seed=seed, decodeNoise=False)
    assert ck.genCryptoContextAndKeyGen() == 1
    return ck


@pytest.fixture(scope="module")
def cfg2(tmp_path_factory):
    return _make(tmp_path_factory, "wide_cfg2", 16384, 3, 7)  # 2^15, L4


@pytest.fixture(scope="module")
def cfg4(tmp_path_factory):
    return _make(tmp_path_factory, "wide_cfg4", 32768, 5, 9)  # 2^16, L6


def _arrays(ck):
    inf = ck.info()
    return (np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64), inf["ring_dim"],
            inf["batch"], inf["delta"])


def _Q(q):
    Q = 1
    for v in q:
        Q *= int(v)
    return Q


W127 = 2.0 ** 127  # the fast CRT's range


def _coeff_range(cts, sk, q, psi, S, scale):
    """(largest |X|, number of coefficients with |X| >= 2^127) over the ciphertexts [K][2][L][N], from
    the oracle's exact centred decrypt (re, im = X / scale as doubles: 53 bits of X, plenty to place
    it against 2^127 -- no case below comes within 2^-10 relative of the boundary)."""
    mx, wide = 0.0, 0
    for ct in cts:
        re, im = O.decrypt_coeffs(ct, sk, q, psi, S, scale)
        a = np.abs(np.concatenate([re, im])) * scale
        mx = max(mx, float(a.max()))
        wide += int((a >= W127).sum())
    return mx, wide


class _Redo:
    """with _Redo(ck, n): the decrypt calls inside were redone exactly n times in all."""

    def __init__(self, ck, n):
        self.ck, self.n = ck, n

    def __enter__(self):
        self.n0 = self.ck.decode_redo_count()

    def __exit__(self, et, ev, tb):
        if et is None:
            assert self.ck.decode_redo_count() - self.n0 == self.n


@pytest.mark.parametrize("cfg", ["cfg2", "cfg4"])
@pytest.mark.parametrize("e", [80, 120])
def test_fresh_wide_values(cfg, e, request):
    """Fresh |x| = 2^e of random sign.  e = 80: |X| ~ 2^126, below 2^127 -- the fast path decodes it
    (no redo); e = 120: redone exactly."""
    ck = request.getfixturevalue(cfg)
    q, psi, N, S, delta = _arrays(ck)
    _, sk = ck.get_keys()
    assert (2.0 ** e) * delta < _Q(q) / 2 ** 3  # inside the reference's range, beyond 2^127
    wide = e == 120
    rng = np.random.default_rng(e)
    x = rng.uniform(-1, 1, S + 5) * 2.0 ** e
    x[3] = 2.0 ** e
    # bytes API
    ck.set_seed(70 + e)
    blob = ck.encrypt(x)
    res = m.blob_residues(blob, N, len(q))
    mx, nw = _coeff_range(res, sk, q, psi, S, delta)
    assert (mx >= W127) == wide and (nw > 0) == wide, mx
    with _Redo(ck, int(wide)):
        dec = ck.decrypt(blob, len(x))
    ref = O.decrypt_vector(res, sk, q, psi, S, delta, len(x))
    assert np.array_equal(dec, ref)
    assert np.abs(dec - x).max() <= 2.0 ** -36 * 2.0 ** e
    # device API (same ciphertexts, uploaded; and a device-side encrypt)
    ct = torch.from_numpy(res.view(np.int64)).cuda()
    with _Redo(ck, int(wide)):
        dd = D.decrypt(ck, ct, len(x), delta).cpu().numpy()
    assert np.array_equal(dd, ref)
    ck.set_seed(90 + e)
    ct2 = D.encrypt(ck, torch.from_numpy(x).cuda())
    r2 = ct2.cpu().numpy().view(np.uint64)
    assert (_coeff_range(r2, sk, q, psi, S, delta)[0] >= W127) == wide
    with _Redo(ck, int(wide)):
        dd2 = D.decrypt(ck, ct2, len(x), delta).cpu().numpy()
    ref2 = O.decrypt_vector(r2, sk, q, psi, S, delta, len(x))
    assert np.array_equal(dd2, ref2)
    assert np.abs(dd2 - x).max() <= 2.0 ** -36 * 2.0 ** e


# (|x|, weights): |sum w x| ~ 2^23 (random signs: |X| ~ 2^121, the fast path), 2^60, 2^100
AGG = {
    23: (1e12, [2.0 ** -18, 2.0 ** -19, 2.0 ** -20, 2.0 ** -19]),
    60: (1e12 * 2.0 ** 20, [0.4, 0.3, 0.2, 0.1]),
    100: (1e12 * 2.0 ** 60, [0.4, 0.3, 0.2, 0.1]),
}


def _learners(S, xm, seed):
    rng = np.random.default_rng(seed)
    sign = rng.choice([-1.0, 1.0], S)
    # same sign per slot across learners: the sum keeps its magnitude
    return [sign * rng.uniform(0.9, 1.0, S) * xm for _ in range(4)]


@pytest.mark.parametrize("cfg", ["cfg2", "cfg4"])
@pytest.mark.parametrize("tb", sorted(AGG))
def test_aggregate_wide_values(cfg, tb, request):
    """Aggregates of random-sign slots.  tb = 23: |X| ~ 2^121, the fast path (no redo); 60, 100:
    redone exactly."""
    ck = request.getfixturevalue(cfg)
    q, psi, N, S, delta = _arrays(ck)
    _, sk = ck.get_keys()
    xm, w = AGG[tb]
    wide = tb != 23
    xs = _learners(S, xm, tb)
    exp = sum(float(np.float32(wi)) * x for wi, x in zip(w, xs))
    assert 2.0 ** (tb - 1) < np.abs(exp).max() < 2.0 ** (tb + 1)
    assert np.abs(exp).max() * delta * delta < _Q(q) / 2 ** 3
    # bytes API
    ck.set_seed(500 + tb)
    blobs = [ck.encrypt(x) for x in xs]
    agg = ck.computeWeightedAverage(blobs, w)
    ar = m.blob_residues(agg, N, len(q))
    mx, nw = _coeff_range(ar, sk, q, psi, S, delta * delta)
    assert (mx >= W127) == wide and (nw > 0) == wide, mx
    with _Redo(ck, int(wide)):
        dec = np.asarray(ck.decrypt(agg, S))
    ref = O.decrypt_vector(ar, sk, q, psi, S, delta * delta, S)
    assert np.array_equal(dec, ref)
    assert np.abs(dec - exp).max() <= 2.0 ** -30 * np.abs(exp).max()
    # device API: encrypt, wavg and decrypt resident in HBM
    ck.set_seed(600 + tb)
    cts = [D.encrypt(ck, torch.from_numpy(x).cuda()) for x in xs]
    dagg = D.wavg(ck, cts, w)
    dr = dagg.cpu().numpy().view(np.uint64)
    assert (_coeff_range(dr, sk, q, psi, S, delta * delta)[0] >= W127) == wide
    with _Redo(ck, int(wide)):
        dd = D.decrypt(ck, dagg, S, delta * delta).cpu().numpy()
    dref = O.decrypt_vector(dr, sk, q, psi, S, delta * delta, S)
    assert np.array_equal(dd, dref)
    assert np.abs(dd - exp).max() <= 2.0 ** -30 * np.abs(exp).max()


def test_mixed_call_only_some_ciphertexts_wide(cfg2):
    """A 3-ciphertext call whose middle ciphertext alone is wide: the redo decodes every
    ciphertext over all towers, and the narrow ones keep the fast path's bits."""
    ck = cfg2
    q, psi, N, S, delta = _arrays(ck)
    _, sk = ck.get_keys()
    x = np.random.default_rng(3).uniform(-1, 1, 3 * S)
    x[S:2 * S] *= 2.0 ** 90
    ck.set_seed(33)
    blob = ck.encrypt(x)
    res = m.blob_residues(blob, N, len(q))
    assert [_coeff_range(res[k:k + 1], sk, q, psi, S, delta)[0] >= W127 for k in range(3)] == [False, True, False]
    with _Redo(ck, 1):
        dec = ck.decrypt(blob, len(x))
    assert np.array_equal(dec, O.decrypt_vector(res, sk, q, psi, S, delta, len(x)))
    with _Redo(ck, 0):
        narrow = ck.decrypt(m.blob_pack(ck, res[[0, 2]]), 2 * S)
    assert np.array_equal(dec[:S], narrow[:S]) and np.array_equal(dec[2 * S:], narrow[S:])


def test_flooded_decode_on_the_fast_path_of_a_large_aggregate(cfg2):
    """Flooding a 2^23 aggregate of random-sign slots (|X| ~ 2^121: the fast path, no redo): the
    noise stream, sigma and logError are the ones the oracle's or_decrypt_flood computes."""
    ck = cfg2
    q, psi, N, S, delta = _arrays(ck)
    _, sk = ck.get_keys()
    xm, w = AGG[23]
    xs = _learners(S, xm, 23)
    seed = 777
    ck.set_seed(seed)
    blobs = [ck.encrypt(x) for x in xs]  # counters 0 .. 3
    agg = ck.computeWeightedAverage(blobs, w)
    ar = m.blob_residues(agg, N, len(q))
    mx, nw = _coeff_range(ar, sk, q, psi, S, delta * delta)
    assert mx < W127 and nw == 0, mx
    with _Redo(ck, 0):
        exact = np.asarray(ck.decrypt(agg, S))
    ck.set_decode_noise(True)
    try:
        with _Redo(ck, 0):
            fl = np.asarray(ck.decrypt(agg, S))  # counter 4
        prec = ck.last_log_precision()
    finally:
        ck.set_decode_noise(False)
    ref, le, fail = O.decrypt_flood(ar[0], sk, q, psi, S, delta * delta, S, seed=seed, g=4)
    assert not fail
    noise = np.abs(fl - exact).max()
    assert noise > 0
    assert np.abs(fl - ref).max() <= 1e-9 * noise
    assert prec == 52 - le


def _flooded_failure(ck, e, wide):
    """A flooded decrypt of fresh |x| = 2^e values that the oracle's Decode refuses: the product
    raises too, after `wide` redos."""
    q, psi, N, S, delta = _arrays(ck)
    _, sk = ck.get_keys()
    x = np.random.default_rng(8).uniform(-1, 1, S) * 2.0 ** e
    ck.set_seed(808)
    blob = ck.encrypt(x)
    res = m.blob_residues(blob, N, len(q))
    assert (_coeff_range(res, sk, q, psi, S, delta)[0] >= W127) == bool(wide)
    _, _, fail = O.decrypt_flood(res[0], sk, q, psi, S, delta, S, seed=808, g=1)
    assert fail
    n0 = ck.decode_redo_count()
    ck.set_decode_noise(True)
    try:
        with pytest.raises(RuntimeError, match="approximation error is too high"):
            ck.decrypt(blob, S)
    finally:
        ck.set_decode_noise(False)
    assert ck.decode_redo_count() - n0 == wide


def test_flooded_decode_failure_on_the_fast_path(cfg2):
    """Fresh 2^80 values carry the encode's 2^18-sized rounding: PALISADE's Decode estimates that
    error and throws; so does the oracle, and so does the product -- on the fast path (|X| ~ 2^126,
    no redo)."""
    _flooded_failure(cfg2, 80, 0)


def test_flooded_decode_failure_after_the_redo(cfg2):
    """The same with fresh 2^120 values (|X| ~ 2^166): the failure is the exact pass's verdict."""
    _flooded_failure(cfg2, 120, 1)


def _positive_learners(S, tb, seed, K=1):
    """4 learners of K S positive slots uniform(0.9, 1.0) 2^tb: the weighted mean lands in each
    ciphertext's constant coefficient, ~0.95 2^tb Delta^2."""
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.9, 1.0, K * S) * 2.0 ** tb for _ in range(4)]


W4 = [0.4, 0.3, 0.2, 0.1]


@pytest.mark.parametrize("api", ["bytes", "device"])
@pytest.mark.parametrize("cfg", ["cfg2", "cfg4"])
@pytest.mark.parametrize("tb", [24, 35])
def test_positive_aggregate_decodes_after_the_redo(tb, cfg, api, request):
    """Aggregates of positive slots ~2^24 (|X_0| ~ 2^127.9: one coefficient past the fast range)
    and ~2^35 (|X_0| ~ 2^138.9).  Unflooded: the oracle's bits.  Flooded -- the default mode -- after
    the redo: ciphertexts the oracle's Decode accepts decode without an exception, with the oracle's
    noise stream, sigma and logError.  (The fast pass's wrapped values do not trip its precision
    test here: the constant coefficient is not in the statistic, and the other wide coefficients come
    in pairs whose wraps cancel -- test_flooded_redo_verdict_is_the_exact_pass_alone has one that
    does not.)"""
    ck = request.getfixturevalue(cfg)
    q, psi, N, S, delta = _arrays(ck)
    _, sk = ck.get_keys()
    xs = _positive_learners(S, tb, tb)
    exp = sum(float(np.float32(wi)) * x for wi, x in zip(W4, xs))
    seed = 900 + tb
    ck.set_seed(seed)  # the encryptions take counters 0 .. 3, the flooded decrypt counter 4
    if api == "bytes":
        agg = ck.computeWeightedAverage([ck.encrypt(x) for x in xs], W4)
        ar = m.blob_residues(agg, N, len(q))

        def dec():
            return np.asarray(ck.decrypt(agg, S))
    else:
        dagg = D.wavg(ck, [D.encrypt(ck, torch.from_numpy(x).cuda()) for x in xs], W4)
        ar = dagg.cpu().numpy().view(np.uint64)

        def dec():
            return D.decrypt(ck, dagg, S, delta * delta).cpu().numpy()
    mx, nw = _coeff_range(ar, sk, q, psi, S, delta * delta)
    assert 2.0 ** (tb + 103) <= mx < 2.0 ** (tb + 104) and mx >= W127, mx
    assert nw == 1 if tb == 24 else nw > 1, nw
    with _Redo(ck, 1):
        exact = dec()
    assert np.array_equal(exact, O.decrypt_vector(ar, sk, q, psi, S, delta * delta, S))
    assert np.abs(exact - exp).max() <= 2.0 ** -30 * np.abs(exp).max()
    ref, le, fail = O.decrypt_flood(ar[0], sk, q, psi, S, delta * delta, S, seed=seed, g=4)
    assert not fail
    ck.set_decode_noise(True)
    try:
        with _Redo(ck, 1):
            fl = dec()
        prec = ck.last_log_precision()
    finally:
        ck.set_decode_noise(False)
    noise = np.abs(fl - exact).max()
    assert noise > 0
    assert np.abs(fl - ref).max() <= 1e-9 * noise
    assert prec == 52 - le


def test_flooded_mixed_call_keeps_each_noise_stream(cfg2):
    """A flooded 3-ciphertext aggregate whose middle ciphertext alone is wide (positive slots
    ~2^35; the outer ones uniform(-1, 1)): after the redo ciphertext k carries the oracle's flooding
    with counter g0 + k, and the call's logError is the largest of the three."""
    ck = cfg2
    q, psi, N, S, delta = _arrays(ck)
    _, sk = ck.get_keys()
    rng = np.random.default_rng(35)
    xs = []
    for _ in range(4):
        x = rng.uniform(-1, 1, 3 * S)
        x[S:2 * S] = rng.uniform(0.9, 1.0, S) * 2.0 ** 35
        xs.append(x)
    seed = 935
    ck.set_seed(seed)
    agg = ck.computeWeightedAverage([ck.encrypt(x) for x in xs], W4)  # counters 0 .. 11
    ar = m.blob_residues(agg, N, len(q))
    assert [_coeff_range(ar[k:k + 1], sk, q, psi, S, delta * delta)[0] >= W127 for k in range(3)] == [False, True, False]
    with _Redo(ck, 1):
        exact = np.asarray(ck.decrypt(agg, 3 * S))
    assert np.array_equal(exact, O.decrypt_vector(ar, sk, q, psi, S, delta * delta, 3 * S))
    refs = [O.decrypt_flood(ar[k], sk, q, psi, S, delta * delta, S, seed=seed, g=12 + k) for k in range(3)]
    assert not any(f for _, _, f in refs)
    ck.set_decode_noise(True)
    try:
        with _Redo(ck, 1):
            fl = np.asarray(ck.decrypt(agg, 3 * S))  # counters 12 .. 14
        prec = ck.last_log_precision()
    finally:
        ck.set_decode_noise(False)
    for k, (ref, _, _) in enumerate(refs):
        sl = slice(k * S, (k + 1) * S)
        noise = np.abs(fl[sl] - exact[sl]).max()
        assert noise > 0
        # the noise within 1e-9 of its own size, as above; on the outer ciphertexts (values ~1, noise
        # ~1e-11) that is below the values' last bit, and value + noise is rounded once more: an ulp
        assert np.abs(fl[sl] - ref).max() <= 1e-9 * noise + 2.0 ** -52 * np.abs(ref).max(), k
    assert prec == 52 - max(le for _, le, _ in refs)


@pytest.mark.parametrize("api", ["bytes", "device"])
def test_flooded_redo_verdict_is_the_exact_pass_alone(cfg2, api):
    """The flooding's statistic is the anti-symmetric part re_i + im_{S-i} of the decrypted
    coefficients, ~0 for a real plaintext.  When both members of a pair are wide they wrap by -+2^128
    in the fast pass and the wrap cancels in it (why the aggregates above never met a false failure);
    a pair that straddles the range does not cancel: re_i = 2^127 + 12345 wraps, im_{S-i} =
    -(2^127 - 54321) does not, and the fast pass sees an error of 2^128.  Its precision failure must
    not outlive it: the oracle's Decode accepts this ciphertext, so the redone call returns the
    oracle's flooded values and logError.  Built with c1 = 0, c0 = NTT of the chosen coefficients (a
    real plaintext's pattern re_j = -im_{S-j} up to 2^20-sized errors, |X| < 2^100 elsewhere)."""
    ck = cfg2
    q, psi, N, S, delta = _arrays(ck)
    _, sk = ck.get_keys()
    rng = np.random.default_rng(127)
    X = [0] * N
    for j in range(1, S):
        r = int.from_bytes(rng.bytes(12), "little") * (1 if j % 3 else -1)  # |r| < 2^96
        X[j] = r
        X[N // 2 + S - j] = -r + int(rng.integers(-(1 << 20), 1 << 20))
    i = 777
    X[i] = (1 << 127) + 12345
    X[N // 2 + S - i] = -((1 << 127) - 54321)
    res = np.zeros((1, 2, len(q), N), np.uint64)
    for t in range(len(q)):
        res[0, 0, t] = O.ntt_fwd(np.array([x % int(q[t]) for x in X], np.uint64), int(q[t]), int(psi[t]))
    # one wide coefficient, counted on the integers (a double cannot tell 2^127 - 54321 from 2^127)
    assert _coeff_range(res, sk, q, psi, S, delta)[0] >= W127
    assert sum(1 for x in X if not -(1 << 127) <= x < 1 << 127) == 1
    seed = 1270
    ref, le, fail = O.decrypt_flood(res[0], sk, q, psi, S, delta, S, seed=seed, g=0)
    assert not fail
    ct = m.blob_pack(ck, res) if api == "bytes" else torch.from_numpy(res.view(np.int64)).cuda()

    def dec():
        if api == "bytes":
            return np.asarray(ck.decrypt(ct, S))
        return D.decrypt(ck, ct, S, delta).cpu().numpy()
    with _Redo(ck, 1):
        exact = dec()
    assert np.array_equal(exact, O.decrypt_vector(res, sk, q, psi, S, delta, S))
    ck.set_seed(seed)  # the flooded decrypt takes counter 0
    ck.set_decode_noise(True)
    try:
        with _Redo(ck, 1):
            fl = dec()
        prec = ck.last_log_precision()
    finally:
        ck.set_decode_noise(False)
    # values ~2^75 / sqrt(S) and more, noise ~2^-45: the noise is below the values' last bit, so the
    # flooded values are the oracle's up to the one rounding of value + noise
    assert np.abs(fl - ref).max() <= 2.0 ** -52 * np.abs(ref).max()
    assert prec == 52 - le


def test_exact_mode(cfg2):
    """set_decode_exact(True) (shelfi_set_decode_exact): every decrypt over every tower through the
    exact CRT.  Same bits as the default on narrow and wide ciphertexts (bytes and device API), and
    the true value of a ciphertext the prefix cannot see: coefficient 0 raised by 7 Q' (Q' = q0 q1
    q2, the default path's prefix) leaves the prefix residues unchanged, while X_0 ~ 2^167 < Q/2.
    Calls in exact mode have no fast pass and leave the redo count alone."""
    ck = cfg2
    q, psi, N, S, delta = _arrays(ck)
    _, sk = ck.get_keys()
    x = np.random.default_rng(11).uniform(-1, 1, 2 * S)
    x[S:] *= 2.0 ** 90
    ck.set_seed(111)
    blob = ck.encrypt(x)
    res = m.blob_residues(blob, N, len(q))
    assert [_coeff_range(res[k:k + 1], sk, q, psi, S, delta)[0] >= W127 for k in range(2)] == [False, True]
    with _Redo(ck, 1):
        a = ck.decrypt(blob, 2 * S)
    Qp = int(q[0]) * int(q[1]) * int(q[2])
    mod = res[:1].copy()
    for t in range(len(q)):  # EVAL domain: a constant polynomial is that constant at every point
        mod[0, 0, t, :] = (mod[0, 0, t, :] + np.uint64(7 * Qp % int(q[t]))) % q[t]
    ck.set_decode_exact(True)
    try:
        with _Redo(ck, 0):
            b = ck.decrypt(blob, 2 * S)
            bd = D.decrypt(ck, torch.from_numpy(res.view(np.int64)).cuda(), 2 * S, delta).cpu().numpy()
            e = ck.decrypt(m.blob_pack(ck, mod), S)
    finally:
        ck.set_decode_exact(False)
    assert np.array_equal(a, b) and np.array_equal(bd, a)
    assert np.array_equal(a, O.decrypt_vector(res, sk, q, psi, S, delta, 2 * S))
    assert np.array_equal(e, O.decrypt_vector(mod, sk, q, psi, S, delta, S))
    assert np.abs(e - x[:S]).max() > 2.0 ** 100  # the 7 Q' term is in the decode
