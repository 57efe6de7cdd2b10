"""Complex slot packing on the MI355X: two values a slot.  Everything is exact equality
against tests/complex_ref.py (the oracle's FFTs, NTTs, encrypt and decrypt around the restated encode;
checked for meaning by tests/test_complex_ref.py), and every output buffer starts filled with ones.

  encode    device.encode (1 tower) against encode_complex: rings 2^11 .. 2^17 at full packing, 2^15 at
            gaps 2 and 4, the smallest batch (from-x fft_inv_blocks), n in {1, 2, V - 1, V, V + 1, 2 V + 3};
            K = 128 at 2^15 (fft_inv_whole); SHELFI_FFT_CT=0 in a child process; imaginary parts that alone
            force the large-value path, through device.encrypt
  encrypt   device.encrypt and encrypt_seeded under set_seed against O.encrypt / the seeded reference of the
            restated plaintext, rings 2^11, 2^13, 2^15, n = V + 1
  decrypt   device.decrypt against decode_complex, the same rings and n; a tower prefix; K = 128 at 2^15 / L2
            (fft_fwd_whole); decrypt_sum at terms = 2; the real parts equal what real mode returns
  bytes     encrypt -> computeWeightedAverage of 3 learners -> decrypt in the three wire formats and seeded, the
            aggregate equal to real mode's on the same ciphertexts, a call over two upload chunks
  threshold partialDecrypt / fuseDecrypt at P = 2 without noise equals the single-key complex decrypt
  guards    decode noise on: decrypt, fuseDecrypt and device.decrypt raise and write nothing, real mode still
            floods afterwards; an unknown mode; info()["values_per_ct"]"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import complex_ref as X
import oracle as O
import seeded_ref as SR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
IN_CHILD = os.environ.get("SHELFI_FFT_CT") == "0"

# id -> (log2 ring, batch, multDepth): full packing on every ring, 2^15 at gaps 2 and 4, the smallest batch of
# the from-x single pass, and 2^15 / L4 (a tower prefix, the flagship shape)
CASES = {"n%d" % l: (l, 1 << (l - 1), 1) for l in range(11, 18)}
CASES.update({"n15_g2": (15, 1 << 13, 1), "n15_g4": (15, 1 << 12, 1), "n11_b1": (11, 1, 1), "n15_L4": (15, 1 << 14, 3)})
ENC_IDS = ["n%d" % l for l in range(11, 18)] + ["n15_g2", "n15_g4", "n11_b1"]
RT_IDS = ["n11", "n13", "n15"]


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _make(cid, seed, packing="complex", noise=False):
    logn, batch, depth = CASES[cid]
    c = m.CKKS("ckks", batch, 52, "", multDepth=depth, ringDim=1 << logn, seed=seed, decodeNoise=noise,
               slotPacking=packing)
    return c


@functools.lru_cache(maxsize=None)
def ctx(cid):
    seed = 1900 + sorted(CASES).index(cid)
    c = _make(cid, seed)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    pk, sk = c.get_keys()
    S = inf["batch"]
    assert inf["values_per_ct"] == 2 * S and inf["slot_packing"] == "complex" and inf["ring_dim"] == 1 << CASES[cid][0]
    return dict(c=c, seed=seed, inf=inf, q=q, psi=psi, pk=pk, sk=sk, S=S, V=2 * S, N=inf["ring_dim"], L=len(q),
                d=inf["delta"])


def _ns(V):
    return sorted({1, 2, V - 1, V, V + 1, 2 * V + 3} - {0})


def _rng(cid, n):
    return np.random.default_rng([sorted(CASES).index(cid), n])


# --------------------------------------------------------------------------------- encode ----
@pytest.mark.parametrize("cid", ENC_IDS)
def test_encode_bitexact(cid):
    x = ctx(cid)
    c, V, N, S = x["c"], x["V"], x["N"], x["S"]
    for n in _ns(V):
        v = _rng(cid, n).uniform(-1, 1, n)
        K = -(-n // V)
        out = torch.ones((K, 1, N), dtype=torch.int64, device="cuda")
        assert D.encode(c, _f64(v), towers=1, out=out) is out
        ref = X.encode_vector_complex(v, N, S, x["d"], x["q"][:1], x["psi"][:1])
        assert np.array_equal(_u64(out), ref), (cid, n)


def test_encode_whole_vector_kernel():
    """K = 128 at 2^15: fft_inv_whole_cx (one workgroup a vector), the last vector ending on an odd value."""
    x = ctx("n15")
    V, N, S, K = x["V"], x["N"], x["S"], 128
    n = K * V - 5
    v = _rng("n15", n).uniform(-1, 1, n)
    out = torch.ones((K, 1, N), dtype=torch.int64, device="cuda")
    D.encode(x["c"], _f64(v), towers=1, out=out)
    got = _u64(out)
    ref = X.encode_vector_complex(v, N, S, x["d"], x["q"][:1], x["psi"][:1])  # every one of the 128 vectors
    assert ref.shape == got.shape
    for k in range(K):
        assert np.array_equal(got[k], ref[k]), k
    for k0 in (0, 64, 124):  # K = 4 calls take the columns / blocks kernels: the same bits
        part = D.encode(x["c"], _f64(v[k0 * V:(k0 + 4) * V]), towers=1)
        assert np.array_equal(_u64(part), got[k0:k0 + 4]), k0


def test_imaginary_parts_alone_force_the_large_value_path():
    x = ctx("n13")
    c, V, N, S, q, psi = x["c"], x["V"], x["N"], x["S"], x["q"], x["psi"]
    v = _rng("n13", 7).uniform(-1, 1, V + 4)
    v[1::2][5] = 2.0 ** 31  # one imaginary part: |x Delta| about 2^83
    c0, a0 = X.encode_coeffs_complex(X.pairs(v[:V], S), N, S, x["d"])
    assert a0 > 0 and np.abs(v[0::2]).max() <= 1
    before = c.encode_redo_count()
    c.set_seed(x["seed"])
    out = torch.ones((2, 2, x["L"], N), dtype=torch.int64, device="cuda")
    D.encrypt(c, _f64(v), out=out)
    assert c.encode_redo_count() == before + 1
    ref = X.encrypt_vector_complex(v, x["pk"], q, psi, N, S, x["d"], x["seed"])
    assert np.array_equal(_u64(out), ref)
    with pytest.raises(ValueError):  # the plaintext encode has no large-value path
        D.encode(c, _f64(v))


# -------------------------------------------------------------------------------- encrypt ----
def _seeded_ref(v, sk, q, psi, N, S, delta, seed_int, g0, seed_bytes):
    """The symmetric encrypt of n interleaved values as a batch [K][2][L][N]: c1 the call seed's stream
    (tests/seeded_ref.py), c0 = NTT(m + e0) - c1 . s with m the restated plaintext's coefficients and e0 the
    public-key encrypt's at (seed_int, g0 + k)."""
    V, L = 2 * S, len(q)
    K = -(-len(v) // V)
    out = np.zeros((K, 2, L, N), np.uint64)
    for k in range(K):
        co, a = X.encode_coeffs_complex(X.pairs(v[k * V:(k + 1) * V], S), N, S, delta)
        assert a == 0
        me = co + O.sample_encrypt(seed_int, g0 + k, N)[1]
        out[k, 1] = SR.expand(seed_bytes, k, q, N)
        for t in range(L):
            qt = np.uint64(q[t])
            u = O.ntt_fwd(np.mod(me, np.int64(q[t])).astype(np.uint64), int(q[t]), int(psi[t]))
            out[k, 0, t] = (u + qt - X.R.mulmod(out[k, 1, t], sk[t], qt)) % qt
    return out


@pytest.mark.parametrize("cid", RT_IDS)
def test_encrypt_and_seeded_encrypt_bitexact(cid):
    x = ctx(cid)
    c, V, N, S, q, psi, L = x["c"], x["V"], x["N"], x["S"], x["q"], x["psi"], x["L"]
    n = V + 1
    v = _rng(cid, n).uniform(-1, 1, n)
    c.set_seed(x["seed"])
    out = torch.ones((2, 2, L, N), dtype=torch.int64, device="cuda")
    assert D.encrypt(c, _f64(v), out=out) is out
    assert np.array_equal(_u64(out), X.encrypt_vector_complex(v, x["pk"], q, psi, N, S, x["d"], x["seed"]))
    # the symmetric encrypt (_seeded_ref)
    c.set_seed(x["seed"])
    c0, seed = D.encrypt_seeded(c, _f64(v))
    assert seed == SR.call_seed(x["seed"], 0) and c0.shape == (2, L, N)
    ref = _seeded_ref(v, x["sk"], q, psi, N, S, x["d"], x["seed"], 0, seed)
    assert np.array_equal(_u64(c0), ref[:, 0])


# -------------------------------------------------------------------------------- decrypt ----
@functools.lru_cache(maxsize=None)
def _cts(cid):
    """ceil((2 V + 3) / V) ciphertexts of uniform complex slots (three from V = 4), made by the reference."""
    x = ctx(cid)
    v = _rng(cid, 0).uniform(-1, 1, 2 * x["V"] + 3)
    ct = X.encrypt_vector_complex(v, x["pk"], x["q"], x["psi"], x["N"], x["S"], x["d"], x["seed"] + 1)
    return v, ct


@pytest.mark.parametrize("cid", ENC_IDS)
def test_decrypt_bitexact_both_halves(cid):
    x = ctx(cid)
    c, V, S, q, psi, sk = x["c"], x["V"], x["S"], x["q"], x["psi"], x["sk"]
    v, ct = _cts(cid)
    K = ct.shape[0]
    full = X.decode_vector_complex(ct, sk, q, psi, S, x["d"], K * V)
    assert np.abs(full[:len(v)] - v).max() < 1e-8
    dct = _dev(ct)
    # the real parts are what real mode returns for the same ciphertexts
    real = _make(cid, 5, packing="real")
    real.set_keys(x["pk"], sk)
    assert np.array_equal(D.decrypt(real, dct, K * S, x["d"]).cpu().numpy(), full[0::2])
    for n in _ns(V):
        out = torch.ones(n + 2, dtype=torch.float64, device="cuda")
        D.decrypt(c, dct, n, x["d"], out=out[:n])
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], full[:n]), (cid, n)
        assert (got[n:] == 1).all(), (cid, n)  # the n-tail rule: nothing past the last value


def test_decrypt_tower_prefix_and_sum():
    x = ctx("n15_L4")
    c, V, S, q, psi, sk, N = x["c"], x["V"], x["S"], x["q"], x["psi"], x["sk"], x["N"]
    v, ct = _cts("n15_L4")
    n = V + 1
    for l in (4, 2, 1):  # decrypt_level: the first l towers of the same ciphertexts
        cl = np.ascontiguousarray(ct[:2, :, :l])
        out = torch.ones(n, dtype=torch.float64, device="cuda")
        D.decrypt(c, _dev(cl), n, x["d"], out=out)
        assert np.array_equal(out.cpu().numpy(), X.decode_vector_complex(cl, sk, q, psi, S, x["d"], n)), l
    # decrypt_sum at terms = 2: residues that are uint64 sums of two canonical residues
    a, b = ct[:2], ct[1:3]
    tot = (a + b) % q[None, None, :, None]
    out = torch.ones(n, dtype=torch.float64, device="cuda")
    D.decrypt_sum(c, _dev(a + b), 2, n, x["d"], out=out)
    assert np.array_equal(out.cpu().numpy(), X.decode_vector_complex(tot, sk, q, psi, S, x["d"], n))


def test_decrypt_whole_vector_kernel():
    """K = 128 at 2^15 / L2 (the fewest towers): fft_fwd_whole_cx, the last vector ending on an odd value."""
    x = ctx("n15")
    c, V, S, q, psi, sk = x["c"], x["V"], x["S"], x["q"], x["psi"], x["sk"]
    _, ct = _cts("n15")
    K = 128
    big = _dev(ct)[torch.arange(K, device="cuda") % 3].contiguous()
    n = K * V - 5
    out = torch.ones(n + 5, dtype=torch.float64, device="cuda")
    D.decrypt(c, big, n, x["d"], out=out[:n])
    got = out.cpu().numpy()
    one = [X.decode_complex(ct[k], sk, q, psi, S, x["d"]) for k in range(3)]
    for k in range(K):
        ref = one[k % 3][:min(V, n - k * V)]
        assert np.array_equal(got[k * V:k * V + len(ref)], ref), k
    assert (got[n:] == 1).all()


# ------------------------------------------------------------------------------ bytes API ----
@pytest.mark.parametrize("wire", ["shelfi", "packed", "palisade"])
def test_bytes_api_round_trip(wire, tmp_path):
    logn, batch, depth = CASES["n13"]
    d = str(tmp_path) + os.sep
    c = m.CKKS("ckks", batch, 52, d, multDepth=depth, ringDim=1 << logn, seed=31, decodeNoise=False,
               wireFormat=wire, slotPacking="complex")
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    pk, sk = c.get_keys()
    S, V, N, delta = inf["batch"], inf["values_per_ct"], inf["ring_dim"], inf["delta"]
    assert c.wire_format() == wire
    n = V + 1
    rng = np.random.default_rng(13)
    xs = [rng.uniform(-1, 1, n) for _ in range(3)]
    c.set_seed(31)
    blobs = [c.encrypt(v) for v in xs]
    res = [_u64(D.from_blob(c, b)) for b in blobs]
    for i, v in enumerate(xs):  # ciphertexts 2 i, 2 i + 1 of the seeded stream
        assert np.array_equal(res[i], X.encrypt_vector_complex(v, pk, q, psi, N, S, delta, 31, g0=2 * i)), i
    w = [0.5, 0.3, 0.2]
    agg = c.computeWeightedAverage(blobs, w)
    ref = O.wavg(res, w, q, delta)
    assert np.array_equal(_u64(D.from_blob(c, agg)), ref)
    c.set_slot_packing("real")  # the mode touches nothing between the two ends
    assert c.computeWeightedAverage(blobs, w) == agg
    c.set_slot_packing("complex")
    dec = c.decrypt(agg, n)
    assert np.array_equal(dec, X.decode_vector_complex(ref, sk, q, psi, S, delta * delta, n))
    exp = sum(wi * v for wi, v in zip(np.float32(w).astype(np.float64), xs))
    assert np.abs(dec - exp).max() < 1e-7


def test_bytes_api_round_trip_seeded_wire():
    """The seeded wire format: encrypt is the symmetric encrypt inside the bytes pipeline (its offsets into x
    moving by V), the aggregate of seeded inputs is packed."""
    logn, batch, depth = CASES["n13"]
    c = m.CKKS("ckks", batch, 52, "", multDepth=depth, ringDim=1 << logn, seed=33, decodeNoise=False,
               wireFormat="seeded", slotPacking="complex")
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    pk, sk = c.get_keys()
    S, V, N, delta = inf["batch"], inf["values_per_ct"], inf["ring_dim"], inf["delta"]
    assert c.wire_format() == "seeded"
    n = V + 1
    rng = np.random.default_rng(14)
    xs = [rng.uniform(-1, 1, n) for _ in range(3)]
    c.set_seed(33)
    blobs = [c.encrypt(v) for v in xs]
    res = [_u64(D.from_blob(c, b)) for b in blobs]
    for i, v in enumerate(xs):  # ciphertexts 2 i, 2 i + 1 of the seeded stream; the call's seed from its first
        ref = _seeded_ref(v, sk, q, psi, N, S, delta, 33, 2 * i, SR.call_seed(33, 2 * i))
        assert np.array_equal(res[i], ref), i
    w = [0.5, 0.3, 0.2]
    agg = c.computeWeightedAverage(blobs, w)
    ref = O.wavg(res, w, q, delta)
    assert np.array_equal(_u64(D.from_blob(c, agg)), ref)
    c.set_slot_packing("real")
    assert c.computeWeightedAverage(blobs, w) == agg
    c.set_slot_packing("complex")
    dec = c.decrypt(agg, n)
    assert np.array_equal(dec, X.decode_vector_complex(ref, sk, q, psi, S, delta * delta, n))
    assert np.array_equal(c.decrypt(blobs[0], n), X.decode_vector_complex(res[0], sk, q, psi, S, delta, n))
    exp = sum(wi * v for wi, v in zip(np.float32(w).astype(np.float64), xs))
    assert np.abs(dec - exp).max() < 1e-7


def test_bytes_api_over_two_upload_chunks():
    """2^15 / L4: encrypt's 64 MiB chunks hold 32 ciphertexts and decrypt's (three decode towers) 42, so 45
    ciphertexts span two chunks of each, the per-chunk offsets into x and out moving by V."""
    x = ctx("n15_L4")
    c, V, S, q, psi, sk, N = x["c"], x["V"], x["S"], x["q"], x["psi"], x["sk"], x["N"]
    K = 45
    n = K * V - 3
    v = _rng("n15_L4", n).uniform(-1, 1, n)
    c.set_wire_format("shelfi")
    c.set_seed(x["seed"])
    blob = c.encrypt(v)
    res = m.blob_residues(blob, N, x["L"])
    assert res.shape[0] == K
    for k in (0, 31, 32, 44):
        ref = X.encrypt_vector_complex(v[k * V:(k + 1) * V], x["pk"], q, psi, N, S, x["d"], x["seed"], g0=k)
        assert np.array_equal(res[k], ref[0]), k
    dec = c.decrypt(blob, n)
    assert np.array_equal(dec, D.decrypt(c, _dev(res), n, x["d"]).cpu().numpy())
    for k in (0, 41, 42, 44):
        ref = X.decode_complex(res[k], sk, q, psi, S, x["d"])[:min(V, n - k * V)]
        assert np.array_equal(dec[k * V:k * V + len(ref)], ref), k
    assert np.abs(dec - v).max() < 1e-8


# ------------------------------------------------------------------------------ threshold ----
def test_threshold_fusion_equals_the_single_key_decrypt():
    cs = [_make("n13", s) for s in (41, 42)]
    assert cs[0].genCryptoContextAndKeyGen() == 1
    pk0, sk0 = cs[0].get_keys()
    cs[1].multipartyKeyGen(pk0)
    pk, sk1 = cs[1].get_keys()
    for c, sk in zip(cs, (sk0, sk1)):
        c.set_keys(pk, sk)
        c.set_threshold_noise(0.0)
        c.set_wire_format("shelfi")
    inf = cs[0].info()
    q = np.array(inf["moduli"], np.uint64)
    V = inf["values_per_ct"]
    n = V + 5
    v = np.random.default_rng(3).uniform(-1, 1, n)
    blob = cs[0].encrypt(v)
    parts = [cs[0].partialDecrypt(blob, True), cs[1].partialDecrypt(blob, False)]
    srv = _make("n13", 43)  # never had keys
    fused = srv.fuseDecrypt(parts, n)
    single = _make("n13", 44)
    single.set_keys(pk, (sk0 + sk1) % q[:, None])
    assert np.array_equal(fused, single.decrypt(blob, n))
    assert np.abs(fused - v).max() < 1e-7
    # the device forms
    ct = D.from_blob(cs[0], blob)
    ps = [D.partial_decrypt(cs[0], ct, True), D.partial_decrypt(cs[1], ct, False)]
    out = torch.ones(n, dtype=torch.float64, device="cuda")
    D.fuse_decrypt(srv, ps, n, inf["delta"], out=out)
    assert np.array_equal(out.cpu().numpy(), fused)


# --------------------------------------------------------------------------------- guards ----
def test_flooded_decode_is_refused_on_complex_slots():
    x = ctx("n11")
    V = x["V"]
    c = _make("n11", 61, noise=True)
    c.set_keys(x["pk"], x["sk"])
    c.set_wire_format("shelfi")
    c.set_threshold_noise(0.0)
    n = V + 1
    v = np.random.default_rng(4).uniform(-1, 1, n)
    blob = c.encrypt(v)
    ct = D.from_blob(c, blob)
    with pytest.raises(RuntimeError, match=r"set_decode_noise\(False\)"):
        c.decrypt(blob, n)
    out = torch.ones(n, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match=r"set_decode_noise\(False\)"):
        D.decrypt(c, ct, n, x["d"], out=out)
    part = c.partialDecrypt(blob, True)
    with pytest.raises(RuntimeError, match=r"set_decode_noise\(False\)"):
        c.fuseDecrypt([part], n)
    with pytest.raises(RuntimeError, match=r"set_decode_noise\(False\)"):
        D.fuse_decrypt(c, [D.partial_decrypt(c, ct, True)], n, x["d"], out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 1).all()  # nothing was written
    assert c.last_log_precision() is None  # shelfi_decode_log_error stays -1
    lib = _lib.load()
    assert lib.shelfi_dev_decrypt(c._ctx, ct.data_ptr(), ct.shape[0], x["d"], n, out.data_ptr(), None) == \
        _lib.SHELFI_ERR_STATE
    # real mode still floods afterwards (a real-packed ciphertext: the imaginary parts it estimates sigma from
    # hold only noise): noisy, close, and with a logError
    c.set_slot_packing("real")
    S = x["S"]
    rblob = c.encrypt(v[:S])
    exact = O.decrypt_vector(_u64(D.from_blob(c, rblob)), x["sk"], x["q"], x["psi"], S, x["d"], S)
    flooded = c.decrypt(rblob, S)
    assert not np.array_equal(flooded, exact) and np.abs(flooded - exact).max() < 1e-6
    assert c.last_log_precision() is not None
    # and with the noise off the complex decode runs
    c.set_slot_packing("complex")
    c.set_decode_noise(False)
    assert np.abs(c.decrypt(blob, n) - v).max() < 1e-8


def test_mode_guards_and_info():
    x = ctx("n11")
    c = _make("n11", 62)
    S = x["S"]
    assert c.info()["values_per_ct"] == 2 * S and c.slot_packing() == "complex"
    c.set_slot_packing("real")
    assert c.info()["values_per_ct"] == S and c.info()["slot_packing"] == "real" and c.slot_packing() == "real"
    with pytest.raises(ValueError):
        c.set_slot_packing("quaternion")
    with pytest.raises(ValueError):
        m.CKKS("ckks", 1024, 52, "", ringDim=2048, slotPacking="both")
    lib = _lib.load()
    for mode in (2, -1):
        assert lib.shelfi_set_slot_packing(c._ctx, mode) == _lib.SHELFI_ERR_ARG
    assert lib.shelfi_get_slot_packing(c._ctx) == 0
    assert m.CKKS("ckks", 1024, 52, "", ringDim=2048).info()["values_per_ct"] == 1024  # the default is real
    # K from the mode: n values take ceil(n / V) ciphertexts, and a short ciphertext batch is refused
    c.set_slot_packing("complex")
    c.set_keys(x["pk"], x["sk"])
    assert D.encrypt(c, torch.zeros(2 * S + 1, dtype=torch.float64, device="cuda")).shape[0] == 2
    one = D.encrypt(c, torch.zeros(2 * S, dtype=torch.float64, device="cuda"))
    assert one.shape[0] == 1
    with pytest.raises(ValueError):
        D.decrypt(c, one, 2 * S + 1, x["d"])
    with pytest.raises(ValueError, match="aligned"):  # a value vector off the 16-byte grid
        D.encrypt(c, torch.zeros(2 * S + 1, dtype=torch.float64, device="cuda")[1:])


# ------------------------------------------------------------------------- SHELFI_FFT_CT=0 ----
@pytest.mark.skipif(IN_CHILD, reason="already the child")
def test_lds_loop_fft_passes_in_a_child_process():
    """SHELFI_FFT_CT=0 (read when a context is created): fft_inv_cols_cx + the LDS-loop fft_inv_blocks, and
    fft_fwd_blocks_cx as a first pass before fft_fwd_cols_cx, on ring 2^15."""
    env = dict(os.environ, SHELFI_FFT_CT="0")
    expr = "(test_encode_bitexact or test_decrypt_bitexact_both_halves) and n15"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-rp", "-p", "no:cacheprovider", "-m", "gpu",
                        os.path.join(HERE, "test_gpu_complex_packing.py"), "-k", expr],
                       env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    passed = [ln for ln in r.stdout.splitlines() if ln.startswith("PASSED")]
    assert any("test_encode_bitexact[n15]" in ln for ln in passed), r.stdout[-3000:]
    assert any("test_decrypt_bitexact_both_halves[n15]" in ln for ln in passed), r.stdout[-3000:]
