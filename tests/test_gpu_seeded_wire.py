"""Seeded ciphertexts on the MI355X: the c1 expansion and the symmetric encrypt bit for
bit against tests/seeded_ref.py (checked for meaning on the CPU by tests/test_seeded_ref.py), the version-3
blob's layout, and every entry that takes ciphertext bytes -- computeWeightedAverage, decrypt, Arena.put,
device.from_blob -- bit-identical to the same ciphertexts re-sent in the packed format, at chunk seams too;
the refusals.

The decrypt bound is tests/test_seeded_ref.py's: a slot's error is a sum of N coefficient errors, each at
most T + 1/2 (|e| <= T = len(gauss_cdt), the encode's rounding), over Delta: N (T + 1) / Delta + 1e-12."""
import functools

import numpy as np
import pytest

import arena_layout as AL
import encode_edge_inputs as E
import oracle as O
import seeded_ref as R
from conftest import PALISADE_DIR, set_switch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

SEED = 77


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _x(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def keyed(name):
    """A context of an encode_edge_inputs shape with keys from keygen(seed); its chain is the oracle's."""
    args, kw = E.ckks_args(name, "")
    ck = m.CKKS(*args, seed=5, decodeNoise=False, **kw)
    assert ck.genCryptoContextAndKeyGen() == 1
    ch = E.chain(name)
    inf = ck.info()
    assert (inf["ring_dim"], inf["batch"], inf["delta"]) == (ch.N, ch.S, ch.delta)
    assert np.array_equal(np.array(inf["moduli"], np.uint64), ch.q)
    return ck, ch, ck.get_keys()[1]


@functools.lru_cache(maxsize=None)
def pal():
    ck = m.CKKS("ckks", 4096, 52, PALISADE_DIR, seed=42, decodeNoise=False)
    ck.loadCryptoParams()
    inf = ck.info()
    q = np.array(inf["moduli"], np.uint64)
    ch = E.Chain(inf["ring_dim"], inf["batch"], inf["num_towers"], q, np.array(inf["roots"], np.uint64), inf["delta"])
    assert ch.N == 8192
    return ck, ch, ck.get_keys()[1]


def _ctx(which):
    return pal() if which == "palisade-keys" else keyed(which)


def _bound(ch):
    return ch.N * (len(O.gauss_cdt()) + 1) / ch.delta + 1e-12


def _seed_of(blob):
    return bytes(blob[64:96])


# ----------------------------------------------------------------- 1. expansion ----
def _c0_pattern(K, l, N):
    return torch.arange(K * l * N, dtype=torch.int64, device="cuda").view(K, l, N)


@pytest.mark.parametrize("name", ["2^11/L2", "2^12/L2", "2^13/L2", "30-bit", "41-bit/2^13"])
@pytest.mark.parametrize("k0", [0, 5])
def test_expand_whole_rings(name, k0):
    ck, ch, _ = keyed(name)
    seed = bytes(range(7, 39))
    c0 = _c0_pattern(3, ch.L, ch.N)
    got = _u64(D.expand_seeded(ck, c0, seed, k0=k0))
    assert got.shape == (3, 2, ch.L, ch.N)
    assert np.array_equal(got[:, 0], _u64(c0))
    for k in range(3):
        assert np.array_equal(got[k, 1], R.expand(seed, k0 + k, ch.q, ch.N)), k


@pytest.mark.parametrize("name", ["2^15/L4", "2^17/L2"])
def test_expand_large_rings_on_sampled_blocks(name):
    ck, ch, _ = keyed(name)
    seed = bytes(range(100, 132))
    K, k0, nb = 3, 2, ch.N // 4
    got = _u64(D.expand_seeded(ck, _c0_pattern(K, ch.L, ch.N), seed, k0=k0))
    blocks = sorted({0, 1, nb - 2, nb - 1} | set(range(0, nb, 257)))
    for k in (0, K - 1):
        for t in range(ch.L):
            assert (got[k, 1, t] < ch.q[t]).all()
            for b, ref in R.expand_blocks(seed, k0 + k, t, ch.q[t], blocks).items():
                assert [int(v) for v in got[k, 1, t, 4 * b:4 * b + 4]] == ref, (k, t, b)


def test_expand_a_tower_prefix():
    ck, ch, _ = keyed("2^13/L2")
    seed = bytes(range(32))
    got = _u64(D.expand_seeded(ck, _c0_pattern(2, 1, ch.N), seed, k0=1))
    assert got.shape == (2, 2, 1, ch.N)
    for k in range(2):
        assert np.array_equal(got[k, 1], R.expand(seed, 1 + k, ch.q[:1], ch.N))
    ck4, ch4, _ = keyed("2^15/L4")
    got = _u64(D.expand_seeded(ck4, _c0_pattern(1, 3, ch4.N), seed))
    full = _u64(D.expand_seeded(ck4, _c0_pattern(1, 4, ch4.N), seed))
    assert np.array_equal(got[0, 1], full[0, 1, :3])


def test_expand_guards():
    ck, ch, _ = keyed("2^13/L2")
    c0 = _c0_pattern(1, ch.L, ch.N)
    with pytest.raises(ValueError):
        D.expand_seeded(ck, c0, b"short")
    with pytest.raises(ValueError):
        D.expand_seeded(ck, c0, bytes(32), k0=1 << 48)
    with pytest.raises(ValueError):
        D.expand_seeded(ck, _c0_pattern(1, ch.L + 1, ch.N), bytes(32))
    D.expand_seeded(ck, c0, bytes(32), k0=(1 << 48) - 1)


# --------------------------------------------------------- 2. symmetric encrypt ----
def _ref_c0(ch, sk, x, seed_int, g0, seed):
    K = -(-len(x) // ch.S)
    return np.stack([R.encrypt_seeded(x[k * ch.S:(k + 1) * ch.S], sk, seed_int, g0 + k, seed, k, ch.N, ch.S, ch.delta,
                                      ch.q, ch.psi)[0] for k in range(K)])


ENC_SHAPES = ["2^11/L2", "2^12/L2", "2^13/L2", "2^15/L4", "2^17/L2", "2^15/gap2", "2^15/gap4", "30-bit"]


@pytest.mark.parametrize("name", ENC_SHAPES)
def test_encrypt_seeded_bitexact(name):
    ck, ch, sk = keyed(name)
    x = np.random.default_rng(len(name)).uniform(-1, 1, ch.S + ch.S // 3)  # K = 2, the second partial
    ck.set_seed(SEED)
    c0, seed = D.encrypt_seeded(ck, _x(x))
    assert tuple(c0.shape) == (2, ch.L, ch.N) and seed == R.call_seed(SEED, 0)
    assert np.array_equal(_u64(c0), _ref_c0(ch, sk, x, SEED, 0, seed))
    # the next call: its ciphertexts' noise goes on at index 2, its stream restarts at ciphertext 0 of a new seed
    c0b, seedb = D.encrypt_seeded(ck, _x(x[:5]))
    assert seedb == R.call_seed(SEED, 2) != seed
    assert np.array_equal(_u64(c0b), _ref_c0(ch, sk, x[:5], SEED, 2, seedb))
    # the expanded batch decrypts
    ct = D.expand_seeded(ck, c0, seed)
    dec = D.decrypt(ck, ct, len(x), ch.delta).cpu().numpy()
    assert np.abs(dec - x).max() <= _bound(ch)


@pytest.mark.parametrize("name", ["2^13/L2", "2^15/L4"])
def test_encrypt_seeded_range_edge(name):
    ck, ch, sk = keyed(name)
    good = np.random.default_rng(5).uniform(-1, 1, ch.S + 3)

    def exact(x):
        ck.set_seed(SEED)
        c0, seed = D.encrypt_seeded(ck, _x(x))
        assert np.array_equal(_u64(c0), _ref_c0(ch, sk, x, SEED, 0, seed))

    def refused(x):
        with pytest.raises(ValueError):
            D.encrypt_seeded(ck, _x(x))
        exact(good)  # the flag word does not leak into the next call

    exact(E.dense_band(ch.S, ch.delta, 2))  # every coefficient about 0.99 2^61 |cos| or |sin|
    top = E.at_coefficient(ch.N, ch.S, ch.delta, "max_fast")
    assert top.coeff == 2 ** 61
    for sign in (1.0, -1.0):
        exact(E.constant(ch.S, sign * top.c))
    over = E.at_coefficient(ch.N, ch.S, ch.delta, "first_redo")
    assert over.coeff > 2 ** 61
    refused(E.constant(ch.S, over.c))
    refused(np.concatenate([good[:ch.S], E.constant(ch.S, -over.c)]))
    bad = good.copy()
    bad[2] = np.nan
    refused(bad)


def test_encrypt_seeded_across_launch_chains(monkeypatch):
    ck, ch, sk = keyed("2^17/L2")  # 1 MiB of scratch a ciphertext: one chain each at SHELFI_DEV_CHUNK_MIB=1
    x = np.random.default_rng(8).uniform(-1, 1, 2 * ch.S + 9)
    ck.set_seed(SEED)
    c0, seed = D.encrypt_seeded(ck, _x(x))
    set_switch(monkeypatch, "SHELFI_DEV_CHUNK_MIB", "1")
    ck.set_seed(SEED)
    c1, seed1 = D.encrypt_seeded(ck, _x(x))
    assert seed1 == seed and torch.equal(c0, c1)
    ref = R.encrypt_seeded(x[2 * ch.S:], sk, SEED, 2, seed, 2, ch.N, ch.S, ch.delta, ch.q, ch.psi)[0]
    assert np.array_equal(_u64(c1)[2], ref)  # the last chain's ciphertext: its own index in both streams


# ------------------------------------------------------------------ 3. the blob ----
def _enc_seeded(ck, x, seed):
    ck.set_wire_format("seeded")
    if seed is not None:
        ck.set_seed(seed)
    try:
        return ck.encrypt(x)
    finally:
        ck.set_wire_format("shelfi")


@pytest.mark.parametrize("which", ["2^15/L4", "palisade-keys"])
def test_seeded_blob_layout(which):
    ck, ch, sk = _ctx(which)
    x = np.random.default_rng(3).uniform(-1, 1, 2 * ch.S - 17)
    blob = _enc_seeded(ck, x, 11)
    U = AL.widths(ch.q)
    assert len(blob) == 128 + 2 * ch.N * sum(U) // 8 == 128 + 2 * R.packed_poly_bytes(ch.q, ch.N)
    info = m.blob_info(blob)
    assert (info["num_cts"], info["depth"], info["format"]) == (2, 1, "seeded")
    assert int.from_bytes(blob[4:6], "little") == 3 and blob[96:128] == bytes(32)
    seed = _seed_of(blob)
    assert seed == R.call_seed(11, 0)
    assert blob[128:] == R.blob_payload(_ref_c0(ch, sk, x, 11, 0, seed), ch.q, ch.N)
    assert _enc_seeded(ck, x, 11) == blob  # the same set_seed, the same bytes
    try:
        ck.set_seed(0)  # OS entropy per call
        a, b = _enc_seeded(ck, x, None), _enc_seeded(ck, x, None)
    finally:
        ck.set_seed(42)
    assert _seed_of(a) != _seed_of(b) and a[128:] != b[128:]
    # the device unpack: c0 from the payload, c1 from the seed
    ct = _u64(D.from_blob(ck, blob))
    assert np.array_equal(ct[:, 0], _ref_c0(ch, sk, x, 11, 0, seed))
    assert np.array_equal(ct[1, 1], R.expand(seed, 1, ch.q, ch.N))


def test_from_blob_takes_every_library_format():
    ck, ch, _ = keyed("2^13/L2")
    x = np.linspace(-1, 1, ch.S + 5)
    for fmt in ("shelfi", "packed", "palisade"):
        ck.set_wire_format(fmt)
        ck.set_seed(9)
        try:
            blob = ck.encrypt(x)
        finally:
            ck.set_wire_format("shelfi")
        assert np.array_equal(_u64(D.from_blob(ck, blob)), m.blob_residues(blob, ch.N, ch.L, ckks=ck)), fmt


# ------------------------------------------------------------- 4. the bytes API ----
def _as_packed(ck, ch, res, depth=1, scale=None):
    """The ciphertexts `res` [K][2][L][N] re-sent as a packed (version-2) blob."""
    b = m.blob_pack(ck, res, depth=depth, scale=scale)
    return b[:4] + (2).to_bytes(2, "little") + b[6:64] + AL.pack_one(res, ch.q, ch.N).tobytes()


@pytest.mark.parametrize("which", ["2^15/L4", "palisade-keys"])
def test_bytes_api_equals_the_packed_resend(which):
    ck, ch, sk = _ctx(which)
    xs = [np.random.default_rng(20 + i).uniform(-1, 1, 2 * ch.S - 3) for i in range(5)]
    w = [0.1, 0.3, -0.2, 0.5, 0.3]
    sd = [_enc_seeded(ck, x, 100 + i) for i, x in enumerate(xs)]
    res = [_u64(D.from_blob(ck, b)) for b in sd]
    pk = [_as_packed(ck, ch, r) for r in res]
    agg = ck.computeWeightedAverage(sd, w)
    assert int.from_bytes(agg[4:6], "little") == 2
    assert agg == ck.computeWeightedAverage(pk, w)
    assert np.array_equal(m.blob_residues(agg, ch.N, ch.L, ckks=ck), O.wavg(res, w, ch.q, ch.delta))
    n = len(xs[0])
    dec = ck.decrypt(sd[0], n)
    assert np.array_equal(dec, ck.decrypt(m.blob_pack(ck, res[0]), n))
    assert np.abs(dec - xs[0]).max() <= _bound(ch)
    # partialDecrypt reads a seeded blob as it reads its packed resend (no smudging noise: bit for bit)
    ck.set_threshold_noise(0.0)
    try:
        assert ck.partialDecrypt(sd[1], True) == ck.partialDecrypt(pk[1], True)
    finally:
        ck.set_threshold_noise()
    # an empty batch
    e0 = _enc_seeded(ck, np.zeros(0), 1)
    assert len(e0) == 128 and m.blob_info(e0)["num_cts"] == 0 and ck.decrypt(e0, 0).shape == (0,)
    assert m.blob_info(ck.computeWeightedAverage([e0, e0], [0.5, 0.5]))["format"] == "packed"
    ck.set_wire_format("seeded")
    try:  # no learners: the empty aggregate, which is never seeded
        assert m.blob_info(ck.computeWeightedAverage([], []))["format"] == "packed"
    finally:
        ck.set_wire_format("shelfi")


# ---------------------------------------------------------------- 5. refusals ----
def test_refusals():
    ck, ch, _ = keyed("2^13/L2")
    x = np.linspace(-1, 1, 2 * ch.S)
    good = _enc_seeded(ck, x, 300)
    res = _u64(D.from_blob(ck, good))
    packed = _as_packed(ck, ch, res)
    with pytest.raises((ValueError, RuntimeError), match="mix seeded"):
        ck.computeWeightedAverage([good, packed], [0.5, 0.5])
    pad = bytearray(good)
    pad[100] = 1
    trunc = good[:-4]
    forged = bytearray(good)
    forged[16:24] = (1 << 63).to_bytes(8, "little")  # K
    huge = bytearray(good)
    huge[16:24] = (1 << 48).to_bytes(8, "little")
    ar = D.Arena(ck, 2, 2, layout="packed")
    for bad, what in ((bytes(pad), "padding"), (trunc, "length"), (bytes(forged), "2\\^48|length"),
                      (bytes(huge), "2\\^48")):
        with pytest.raises((ValueError, RuntimeError), match=what):
            ck.decrypt(bad, 2 * ch.S)
        with pytest.raises((ValueError, RuntimeError), match=what):
            ck.computeWeightedAverage([good, bad], [0.5, 0.5])
        with pytest.raises((ValueError, RuntimeError), match=what):
            ar.put(0, bad)
        with pytest.raises((ValueError, RuntimeError), match=what):
            D.from_blob(ck, bad, out=D.empty_ct(ck, 2))
    with pytest.raises((ValueError, RuntimeError), match="from_blob"):
        m.blob_residues(good, ch.N, ch.L, ckks=ck)
    out = np.empty((2, 2, ch.L, ch.N), np.uint64)
    import ctypes as C

    rc = m._lib.load().shelfi_blob_unpack(ck._ctx, C.cast(C.c_char_p(good), m._lib.u8p), len(good),
                                          out.ctypes.data_as(m._lib.u64p))
    assert rc != 0 and b"shelfi_dev_blob_unpack" in m._lib.load().shelfi_last_error()
    # a residue field of all ones is >= q_t
    U0 = AL.widths(ch.q)[0]
    ones = bytearray(good)
    ones[128:128 + 64 * U0] = b"\xff" * (64 * U0)
    with pytest.raises(RuntimeError, match="residue >= its tower modulus"):
        ck.computeWeightedAverage([good, bytes(ones)], [0.5, 0.5])
    with pytest.raises(m.ShelfiError, match="residue"):
        ar.put(0, bytes(ones))
    # a context without keys, and one whose secret is a threshold share
    batch, N, depth, sb, fb = E.SHAPES["2^13/L2"]
    bare = m.CKKS("ckks", batch, sb, "", multDepth=depth, firstModBits=fb, ringDim=N, seed=9, decodeNoise=False)
    with pytest.raises(m.ShelfiError) as ei:
        D.encrypt_seeded(bare, _x(x))
    assert ei.value.code == m._lib.SHELFI_ERR_STATE
    bare.set_wire_format("seeded")
    with pytest.raises(m.ShelfiError) as ei:
        bare.encrypt(x)
    assert ei.value.code == m._lib.SHELFI_ERR_STATE
    party = m.CKKS("ckks", batch, sb, "", multDepth=depth, firstModBits=fb, ringDim=N, seed=10, decodeNoise=False)
    party.multipartyKeyGen(ck.get_keys()[0])
    with pytest.raises(m.ShelfiError, match="threshold share") as ei:
        D.encrypt_seeded(party, _x(x))
    assert ei.value.code == m._lib.SHELFI_ERR_STATE
    party.set_wire_format("seeded")
    with pytest.raises(m.ShelfiError, match="threshold share"):
        party.encrypt(x)
    party.set_keys(*ck.get_keys())  # a whole key again
    party.set_wire_format("seeded")
    assert m.blob_info(party.encrypt(x))["format"] == "seeded"
    # the context stays usable
    assert np.abs(ck.decrypt(good, 2 * ch.S) - x).max() <= _bound(ch)


# ------------------------------------------------------------- 6. chunk seams ----
def test_chunk_seams(monkeypatch):
    ck, ch, _ = keyed("2^15/L4")
    K = 5
    xs = [np.random.default_rng(60 + i).uniform(-1, 1, K * ch.S - 11) for i in range(3)]
    w = [0.2, 0.5, 0.3]
    sd = [_enc_seeded(ck, x, 400 + i) for i, x in enumerate(xs)]
    res = [_u64(D.from_blob(ck, b)) for b in sd]
    pk = [_as_packed(ck, ch, r) for r in res]
    n = len(xs[0])
    agg, dec = ck.computeWeightedAverage(sd, w), ck.decrypt(sd[0], n)
    a, b, c = (D.Arena(ck, 3, K, layout="packed") for _ in range(3))
    for i in range(3):
        a.put(i, sd[i])
        c.put(i, pk[i])
    # one ciphertext an aggregation chunk (5 chunks), ring slots smaller than a ciphertext's c0
    for var in ("SHELFI_DEV_CHUNK_MIB", "SHELFI_WAVG_CHUNK_MIB", "SHELFI_STAGE_SLOT_MIB"):
        set_switch(monkeypatch, var, "1")
    assert ck.computeWeightedAverage(sd, w) == agg == ck.computeWeightedAverage(pk, w)
    assert np.array_equal(ck.decrypt(sd[0], n), dec)
    for i in range(3):
        b.put(i, sd[i])
        assert np.array_equal(_u64(D.from_blob(ck, sd[i])), res[i])
    torch.cuda.synchronize()
    assert torch.equal(a.buf, b.buf) and torch.equal(a.buf, c.buf)
    assert torch.equal(a.wavg(w), c.wavg(w))
    assert np.array_equal(_u64(b.wavg(w)), m.blob_residues(agg, ch.N, ch.L, ckks=ck))
    set_switch(monkeypatch, "SHELFI_H2D_DIRECT", "1")  # direct uploads, two threads
    assert ck.computeWeightedAverage(sd, w) == agg


def test_seams_of_the_fixed_upload_chunks():
    """decrypt, partialDecrypt, Arena.put and from_blob upload in chunks of 64 MiB of ciphertexts whatever the
    switches say: 16 ciphertexts at 2^17 / L2, so K = 33 spans three chunks, the last of one ciphertext."""
    ck, ch, _ = keyed("2^17/L2")
    K = 33
    x = np.random.default_rng(70).uniform(-1, 1, K * ch.S - 5)
    blob = _enc_seeded(ck, x, 500)
    seed = _seed_of(blob)
    ct = D.from_blob(ck, blob)
    res = _u64(ct)
    nb = ch.N // 4
    for k in (0, 15, 16, 31, 32):  # each side of each seam: the stream of the ciphertext's index in the blob
        for t in range(ch.L):
            for b, ref in R.expand_blocks(seed, k, t, ch.q[t], [0, 257, nb - 1]).items():
                assert [int(v) for v in res[k, 1, t, 4 * b:4 * b + 4]] == ref, (k, t, b)
    resend = m.blob_pack(ck, res)
    dec = ck.decrypt(blob, len(x))
    assert np.array_equal(dec, ck.decrypt(resend, len(x)))
    assert np.abs(dec - x).max() <= _bound(ch)
    ck.set_threshold_noise(0.0)
    try:
        assert ck.partialDecrypt(blob, False) == ck.partialDecrypt(resend, False)
    finally:
        ck.set_threshold_noise()
    a, b = D.Arena(ck, 1, K, layout="packed"), D.Arena(ck, 1, K, layout="packed")
    a.put(0, blob)
    b.put(0, ct)
    torch.cuda.synchronize()
    assert torch.equal(a.buf, b.buf)
