"""Encode's large-value path on the HIP path (VERDICT r4 missing 1; ckks.cpp:80 ->
CKKSPackedEncoding::Encode's approxFactor): values whose message coefficients
round(FFTSpecialInv(x)_i / S * Delta) exceed 2^61 are no longer refused.  The fast kernels flag such a
coefficient (not |x Delta|: uniform data of amplitude xmax has coefficients near xmax Delta / sqrt(S)
times a few), and the call is redone with per-ciphertext scale-down exponents (encrypt.hip
launch_encrypt_approx); CKKS.encode_redo_count() says whether it was.  Every ciphertext is bit-exact vs
the oracle's restatement (or_encode_coeffs_ex), and decrypts within 2^-40 relative of the input.
tests/test_gpu_encode_edge.py walks the range's edges on every dispatch branch.

Tolerances: a fresh ciphertext decrypts within 2^-40 * max|x|, because the scale-down keeps 62 bits
of every coefficient.  An aggregate decrypts within 2^-38 * max|x|.  Weighted sums beyond the
decode's range wrap, as in the reference: |sum w x| Delta^2 must stay below 2^127 (2^15 / L4:
|x| < 2^23) and below Q / 2 (2^13 / L2: Q ~ 2^113, so |x| < 2^8 for an aggregate).
Parity with PALISADE itself is unpinned (no reference fixture holds such a ciphertext)."""
import os

import numpy as np
import pytest

import oracle as O
from conftest import PALISADE_DIR, set_switch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402


@pytest.fixture(scope="module")
def c2(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("keys_large")) + os.sep
    ck = m.CKKS("ckks", 16384, 52, d, multDepth=3, seed=7, decodeNoise=False)
    assert ck.genCryptoContextAndKeyGen() == 1
    return ck


def _arrays(ck):
    inf = ck.info()
    return (np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64), inf["ring_dim"],
            inf["batch"], inf["delta"])


def _redone(x, N, S, delta):
    """Whether a call encrypting x is redone, and why, from the oracle's encode: (some logApprox > 0,
    the largest |coefficient| over the ciphertexts whose logApprox is 0)."""
    las, top = [], 0
    for k in range(0, len(x), S):
        c, la = O.encode_coeffs_ex(x[k:k + S], N, S, delta)
        las.append(la)
        if la == 0:
            top = max(top, int(np.abs(c).max()))
    return max(las) > 0, top


# What these inputs reach at 2^15 / L4 (max coefficient, exponent; O.encode_coeffs_ex): 2^9.5 -> 2^55.4,
# 2^10 -> 2^55.7, 2^14 -> 2^59.8: all on the fast path, never flagged; 2^16 -> 2^61.8 with logApprox 0
# (the redo that scales nothing down); 2^20 -> logApprox 4; 1e12 -> logApprox 24
REDONE = {2.0 ** 9.5: 0, 2.0 ** 10: 0, 2.0 ** 14: 0, 2.0 ** 16: 1, 2.0 ** 20: 1, 1e12: 1}


@pytest.mark.parametrize("xmax", list(REDONE))
def test_large_values_bitexact_and_decrypt(c2, xmax):
    q, psi, N, S, delta = _arrays(c2)
    redo = REDONE[xmax]
    pk, sk = c2.get_keys()
    rng = np.random.default_rng(int(np.log2(xmax) * 10))
    x = rng.uniform(-xmax, xmax, 3 * S - 11)
    x[S + 7] = xmax
    scaled, top = _redone(x, N, S, delta)
    assert redo == (scaled or top > 2 ** 61)
    if xmax == 2.0 ** 16:
        assert not scaled and top > 2 ** 61
    seed = 900 + int(np.log2(xmax))
    c2.set_seed(seed)
    n0 = c2.encode_redo_count()
    blob = c2.encrypt(x)
    assert c2.encode_redo_count() - n0 == redo
    got = m.blob_residues(blob, N, len(q))
    ref = O.encrypt_vector(x, pk, q, psi, N, S, delta, seed=seed, g0=0)
    assert np.array_equal(got, ref)
    dec = c2.decrypt(blob, len(x))
    assert np.array_equal(dec, O.decrypt_vector(ref, sk, q, psi, S, delta, len(x)))
    assert np.abs(dec - x).max() <= 2.0 ** -40 * xmax


def test_only_some_ciphertexts_scale_down(c2):
    """A call whose middle ciphertext alone holds large values: its exponent differs from its
    neighbours' (0), and the small ciphertexts equal the fast path's residues."""
    q, psi, N, S, delta = _arrays(c2)
    pk, _ = c2.get_keys()
    x = np.random.default_rng(3).uniform(-1, 1, 3 * S)
    x[S:2 * S] *= 2.0 ** 18
    c2.set_seed(31)
    n0 = c2.encode_redo_count()
    got = m.blob_residues(c2.encrypt(x), N, len(q))
    assert c2.encode_redo_count() - n0 == 1
    ref = O.encrypt_vector(x, pk, q, psi, N, S, delta, seed=31, g0=0)
    assert np.array_equal(got, ref)
    small = x.copy()
    small[S:2 * S] = 0.5
    c2.set_seed(31)
    fast = m.blob_residues(c2.encrypt(small), N, len(q))
    assert c2.encode_redo_count() - n0 == 1  # the fast path
    assert np.array_equal(got[0], fast[0]) and np.array_equal(got[2], fast[2])


def test_device_api_and_multichunk_bytes_api(c2):
    """D.encrypt (device-resident) and a 70-ciphertext bytes-API call (3 pipeline chunks) are bit-exact
    vs the oracle.  The device call's third ciphertext has coefficients up to 2^61.9 with logApprox 0:
    redone, once.  The bytes call's one slot of 3e6 spreads to coefficients of 2^59.5 only: the fast
    path, no redo (the chunked redo is test_chunked_bytes_call_is_redone_once)."""
    q, psi, N, S, delta = _arrays(c2)
    pk, _ = c2.get_keys()
    x = np.random.default_rng(4).uniform(-1, 1, 4 * S)
    x[2 * S:3 * S] *= 2.0 ** 16
    c2.set_seed(41)
    n0 = c2.encode_redo_count()
    ct = D.encrypt(c2, torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert c2.encode_redo_count() - n0 == 1
    assert np.array_equal(ct.cpu().numpy().view(np.uint64), O.encrypt_vector(x, pk, q, psi, N, S, delta, seed=41))
    K = 70
    xb = np.random.default_rng(5).uniform(-1, 1, K * S - 3)
    xb[40 * S + 17] = 3.0e6
    c2.set_seed(42)
    got = m.blob_residues(c2.encrypt(xb), N, len(q))
    assert c2.encode_redo_count() - n0 == 1
    for k in (0, 39, 40, 41, 69):
        ref = O.encrypt_vector(xb[k * S:(k + 1) * S], pk, q, psi, N, S, delta, seed=42, g0=k)
        assert np.array_equal(got[k], ref[0]), k


def test_chunked_bytes_call_is_redone_once(c2):
    """70 ciphertexts through the bytes API (3 pipeline chunks of 32) with flagged ciphertexts in the
    second and third chunks: the whole call is redone, and counted once."""
    q, psi, N, S, delta = _arrays(c2)
    pk, _ = c2.get_keys()
    K = 70
    xb = np.random.default_rng(8).uniform(-1, 1, K * S - 3)
    xb[40 * S + 17] = 3.0e8  # logApprox 5
    xb[41 * S:42 * S] *= 2.0 ** 16  # coefficients above 2^61, logApprox 0
    xb[69 * S + 5] = -1e12  # logApprox 16
    las = [O.encode_coeffs_ex(xb[k * S:(k + 1) * S], N, S, delta)[1] for k in (39, 40, 41, 69)]
    assert las[0] == 0 and las[1] > 0 and las[2] == 0 and las[3] > las[1]
    assert _redone(xb[41 * S:42 * S], N, S, delta)[1] > 2 ** 61
    c2.set_seed(43)
    n0 = c2.encode_redo_count()
    got = m.blob_residues(c2.encrypt(xb), N, len(q))
    assert c2.encode_redo_count() - n0 == 1
    for k in (0, 39, 40, 41, 42, 69):
        ref = O.encrypt_vector(xb[k * S:(k + 1) * S], pk, q, psi, N, S, delta, seed=43, g0=k)
        assert np.array_equal(got[k], ref[0]), k


def test_aggregate_of_large_values(c2):
    """computeWeightedAverage of three learners with |x| up to 2^20: the aggregate is bit-exact vs
    the oracle and decrypts to sum (float)w_i x_i (depth 2: |X| ~ 2^124 < 2^127)."""
    q, psi, N, S, delta = _arrays(c2)
    _, sk = c2.get_keys()
    rng = np.random.default_rng(6)
    xs = [rng.uniform(-2.0 ** 20, 2.0 ** 20, 2 * S) for _ in range(3)]
    w = [0.2, 0.3, 0.5]
    c2.set_seed(51)
    n0 = c2.encode_redo_count()
    blobs = [c2.encrypt(x) for x in xs]
    assert c2.encode_redo_count() - n0 == 3
    res = [m.blob_residues(b, N, len(q)) for b in blobs]
    agg = c2.computeWeightedAverage(blobs, w)
    ar = m.blob_residues(agg, N, len(q))
    assert np.array_equal(ar, O.wavg(res, w, q, delta))
    dec = c2.decrypt(agg, 2 * S)
    exp = sum(float(np.float32(wi)) * x for wi, x in zip(w, xs))
    assert np.array_equal(dec, O.decrypt_vector(ar, sk, q, psi, S, delta * delta, 2 * S))
    assert np.abs(dec - exp).max() <= 2.0 ** -38 * 2.0 ** 20


def test_reference_keys_and_refusals():
    """2^13 / L2 with the reference's own keys: 1e9 (|x Delta| ~ 2^82) encrypts and decrypts in
    every wire format; non-finite values are still refused (PALISADE's log2 of inf / nan)."""
    ck = m.CKKS("ckks", 4096, 52, PALISADE_DIR, seed=61, decodeNoise=False)
    ck.loadCryptoParams()
    q, psi, N, S, delta = _arrays(ck)
    pk, _ = ck.get_keys()
    x = np.array([1e9, -3.0, 0.25, -7.5e8])
    for fmt in ("palisade", "shelfi", "packed"):
        ck.set_wire_format(fmt)
        ck.set_seed(62)
        n0 = ck.encode_redo_count()
        b = ck.encrypt(x)
        assert ck.encode_redo_count() - n0 == 1
        assert np.array_equal(m.blob_residues(b, N, len(q), ckks=ck),
                              O.encrypt_vector(x, pk, q, psi, N, S, delta, seed=62))
        assert np.abs(ck.decrypt(b, 4) - x).max() <= 2.0 ** -40 * 1e9
    n0 = ck.encode_redo_count()
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            ck.encrypt(np.array([1e9, bad]))
    assert ck.encode_redo_count() == n0  # a refusal is not a redo


def _encrypt_chunks(inf, K, mib):
    """shelfi_dev_encrypt's launch chains under SHELFI_DEV_CHUNK_MIB = mib: K split evenly over the fewest
    chains whose scratch fits the budget, at encrypt_scratch_bytes(p, 1) (encrypt.hip) per ciphertext: the
    FFT buffer, pbuf [3][L][N], me0 and ve [N], the large-value path's words, and 64."""
    N, S, L = inf["ring_dim"], inf["batch"], inf["num_towers"]
    per = S * 16 + 3 * L * N * 8 + N * 10 + 16 + 16 * L + 64
    cap = max(1, (mib << 20) // per)
    nch = -(-K // cap)
    kc = -(-K // nch)
    return [min(kc, K - k0) for k0 in range(0, K, kc)]


def test_chunked_device_call_is_redone_once(tmp_path, monkeypatch):
    """D.encrypt cut into launch chains (SHELFI_DEV_CHUNK_MIB=1) with the one large value in the last, shorter
    chain: both passes walk the same chunks, so the ciphertexts are bit-identical to the unsplit call's and the
    call is redone, and counted, once; the same split without the large value is not redone.  Ring 2^13 / L2
    with 2048 slots: 496 KiB of scratch a ciphertext, two to the MiB (4096 slots would leave one, and no
    shorter last chain)."""
    ck = m.CKKS("ckks", 2048, 52, str(tmp_path) + os.sep, ringDim=8192, seed=71, decodeNoise=False)
    assert ck.genCryptoContextAndKeyGen() == 1
    inf = ck.info()
    N, S = inf["ring_dim"], inf["batch"]
    assert (N, inf["num_towers"], S) == (8192, 2, 2048)
    # the smallest count cut into at least three chains, the last one shorter
    chunks = next(c for c in (_encrypt_chunks(inf, k, 1) for k in range(3, 64)) if len(c) >= 3 and c[-1] < c[0])
    K = sum(chunks)
    assert chunks == [2, 2, 1] and _encrypt_chunks(inf, K, 4096) == [K]
    n = K * S - 3
    small = np.random.default_rng(9).uniform(-1, 1, n)
    x = small.copy()
    last = (K - chunks[-1]) * S  # the first slot of the last chain
    x[last + 5] = 2.0 ** 24
    scaled, top = _redone(small, N, S, inf["delta"])
    assert not scaled and top <= 2 ** 61  # the earlier chains, and the call without the large value
    scaled, top = _redone(x[last:], N, S, inf["delta"])
    assert scaled or top > 2 ** 61

    def run(v):
        ck.set_seed(72)
        n0 = ck.encode_redo_count()
        ct = D.encrypt(ck, torch.from_numpy(v).cuda())
        torch.cuda.synchronize()
        return ct.cpu().numpy().view(np.uint64).copy(), ck.encode_redo_count() - n0

    whole, redone = run(x)
    assert redone == 1
    set_switch(monkeypatch, "SHELFI_DEV_CHUNK_MIB", "1")
    split, redone = run(x)
    assert redone == 1
    assert np.array_equal(split, whole)
    assert run(small)[1] == 0
    set_switch(monkeypatch, "SHELFI_DEV_CHUNK_MIB", None)
