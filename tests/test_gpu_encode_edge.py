"""Encrypt at the edges of its message-coefficient range, on every dispatch branch of launch_encrypt
(fhe-fed_amd/csrc/encrypt.hip).  The inputs are tests/encode_edge_inputs.py's; that they land where
they claim (coefficients in (2^60, 2^61], exactly 2^61, 2^61 + 512, 2^62 - 512, the wrap, logApprox 1,
logApprox ~950, an infinite scaled value) is checked on the CPU in tests/test_encode_edge_inputs.py,
together with the decode's closeness to x.  Here every case asserts only equalities:
  * the residues equal the oracle's with the same seed;
  * the decrypt equals the oracle's decrypt of them;
  * CKKS.encode_redo_count() moves by exactly 0 (the fast kernels took it: dense_band, the constant at
    2^61) or 1 (a call holding any flagged ciphertext): a test knows which path it ran.

What the fast kernels rely on, and only coefficients near 2^61 stress: red_any's 32-bit quotient
estimate on u = m + e0 + floor(2^62 / q) q up to ~2^62.6 (enc_cols_fused's message_poly, q >= 2^40: the
41-bit contexts are its smallest class), the unreduced upper rows into the first butterfly, the
mod_signed_dev path of ntt_fwd_cols_enc / ntt_fwd_blocks_enc, and the NORED towers' "inputs below 17 q".

BRANCHES names the kernels each row reaches (read off launch_encrypt for that ring, K and switch)."""
import os

import numpy as np
import pytest

import encode_edge_inputs as E
import oracle as O
from conftest import PALISADE_DIR, set_switch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

SEED = 20611
THREADS = 16
PALISADE = "palisade 2^13/L2"  # the reference's own keys; the chain is "2^13/L2"'s

_CTX, _REF = {}, {}


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    """name -> (CKKS, chain, pk, sk), made once per module; the product's chain is the oracle's."""
    def get(name):
        if name not in _CTX:
            if name == PALISADE:
                ck = m.CKKS("ckks", 4096, 52, PALISADE_DIR, seed=61, decodeNoise=False)
                ck.loadCryptoParams()
                ch = E.chain("2^13/L2")
            else:
                d = str(tmp_path_factory.mktemp("keys_edge")) + os.sep
                args, kw = E.ckks_args(name, d)
                ck = m.CKKS(*args, seed=7, decodeNoise=False, **kw)
                assert ck.genCryptoContextAndKeyGen() == 1
                ch = E.chain(name)
            inf = ck.info()
            assert (inf["ring_dim"], inf["batch"], inf["delta"]) == (ch.N, ch.S, ch.delta)
            assert np.array_equal(np.array(inf["moduli"], np.uint64), ch.q)
            assert np.array_equal(np.array(inf["roots"], np.uint64), ch.psi)
            pk, sk = ck.get_keys()
            _CTX[name] = (ck, ch, pk, sk)
        return _CTX[name]

    yield get
    _CTX.clear()
    _REF.clear()


def _oracle(c, x, g0=0):
    """(residues, decrypt) of x from the oracle, seeded as the product."""
    _, ch, pk, sk = c
    ref = O.encrypt_vector_omp(x, pk, ch.q, ch.psi, ch.N, ch.S, ch.delta, seed=SEED, g0=g0, nthreads=THREADS)
    dec = O.decrypt_vector_omp(ref, sk, ch.q, ch.psi, ch.S, ch.delta, len(x), nthreads=THREADS)
    return ref, dec


def _encrypt(c, api, x):
    """-> (handle for _decrypt, residues [K][2][L][N])."""
    ck, ch = c[0], c[1]
    ck.set_seed(SEED)
    if api == "device":
        ct = D.encrypt(ck, torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        return ct, ct.cpu().numpy().view(np.uint64)
    blob = ck.encrypt(x)
    return blob, m.blob_residues(blob, ch.N, ch.L, ckks=ck)


def _decrypt(c, api, h, n):
    ck, ch = c[0], c[1]
    if api == "device":
        return D.decrypt(ck, h, n, ch.delta).cpu().numpy()
    return ck.decrypt(h, n)


def _check(c, api, x, ref, dec, redo):
    ck = c[0]
    n0 = ck.encode_redo_count()
    h, got = _encrypt(c, api, x)
    assert ck.encode_redo_count() - n0 == redo
    assert np.array_equal(got, ref), "residues differ from the oracle"
    assert np.array_equal(_decrypt(c, api, h, len(x)), dec), "decrypt differs from the oracle"
    return got


# ------------------------------------------------- dense_band on every branch ----
# (context, K, switch): the smallest K that reaches the branch
BRANCHES = [
    ("2^11/L2", 2, None),      # enc_prep_kernel; ntt_fwd_blocks_enc<4> reads the compact record, no columns pass
    ("2^12/L2", 2, None),      # enc_prep_kernel + ntt_fwd_cols_enc<1>; ntt_fwd_blocks_enc_ct<11>
    ("2^13/L2", 2, None),      # enc_prep_kernel + ntt_fwd_cols_enc<2>; ntt_fwd_blocks_enc_ct<11>
    ("2^14/L3", 2, None),      # enc_cols_fused<3, true>; ntt_fwd_blocks_enc_pp, one launch
    ("2^14/L3", 2, ("SHELFI_ENC_TAB", "0")),      # enc_cols_fused<3, false>
    ("2^14/L3", 192, None),    # persistent pass split: tower 0 reduced, towers 1-2 NORED
    ("2^14/L3", 192, ("SHELFI_ENC_NORED", "0")),  # persistent pass, reductions in every tower
    ("2^15/L4", 2, None),      # TS: enc_cols_fused<4, true, 3, true, true>, one wave per tower
    ("2^15/L4", 25, None),     # VT: enc_cols_fused<.., false, true>; ntt_fwd_blocks_enc_pp<.., VT>
    ("2^15/L4", 25, ("SHELFI_ENC_VT", "0")),          # v's columns pass in enc_cols_fused<4, true, 3, true>
    ("2^15/L4", 25, ("SHELFI_ENC_TS", "1")),          # TS forced above kEncTsMaxK
    ("2^15/L4", 25, ("SHELFI_ENC_TAB", "0")),         # enc_cols_fused<4, false>
    ("2^15/L4", 25, ("SHELFI_ENC_FUSED_COLS", "0")),  # enc_prep_kernel + ntt_fwd_cols_enc<4>; blocks_enc_ct<11>
    ("2^15/L4", 25, ("SHELFI_ENC_PP", "0")),          # one-shot ntt_fwd_blocks_enc_ct<11>
    ("2^15/L4", 25, ("SHELFI_NTT_WL", "0")),          # workgroup barrier at every block-pass exchange; no VT
    ("2^15/L4", 192, None),    # NORED + VT: tower 0 reduced, towers 1-3 unreduced, both with table sums
    ("2^15/gap2", 2, None),    # fused columns, coefficients that are not slots
    ("2^15/gap4", 2, None),
    ("2^16/L2", 2, None),      # X5: 16 register rows + the exchanged fifth stage; persistent pass
    ("2^16/L2", 2, ("SHELFI_ENC_X5", "0")),           # enc_prep_kernel + ntt_fwd_cols_enc<5>; blocks_enc_ct<11>
    ("2^17/L2", 2, None),      # X5 columns; 2^12 blocks: ntt_fwd_blocks_enc_ct<12>
    ("30-bit", 2, None),       # dt.red_ok false: mod_signed_dev and the generic ntt_fwd_blocks_enc<4>
    ("41-bit/2^13", 2, None),  # 45 / 42-bit towers through ntt_fwd_cols_enc<2>, blocks_enc_ct<11>
    ("41-bit/2^15", 2, None),  # 41-bit tower through red_any in enc_cols_fused (TS)
    ("41-bit/2^15", 25, None),  # ... and through the VT form
]


def _band(c, name, K):
    if (name, K) not in _REF:
        ch = c[1]
        x = E.dense_band(ch.S, ch.delta, K, seed=K)[:K * ch.S - 3]  # a ragged last ciphertext
        _REF[(name, K)] = (x,) + _oracle(c, x)
    return _REF[(name, K)]


@pytest.mark.parametrize("name,K,switch", BRANCHES,
                         ids=["%s-K%d-%s" % (n, k, "default" if s is None else "=".join(s)) for n, k, s in BRANCHES])
def test_dense_band_on_every_branch(ctx, monkeypatch, name, K, switch):
    c = ctx(name)
    if name.startswith("41-bit"):  # red_any's smallest modulus class: 41 or 42 bits, nothing below 2^40
        bits = [int(q).bit_length() for q in c[0].info()["moduli"]]
        assert min(bits) in (41, 42) and bits == ([45, 42] if c[1].L == 2 else [45, 42, 41, 42])
    x, ref, dec = _band(c, name, K)
    if switch is not None:
        set_switch(monkeypatch, *switch)
    _check(c, "device", x, ref, dec, redo=0)


@pytest.mark.parametrize("wire", ["palisade", "packed"])
def test_dense_band_through_the_bytes_api(ctx, wire):
    c = ctx("2^13/L2")
    x, ref, dec = _band(c, "2^13/L2", 2)
    c[0].set_wire_format(wire)
    try:
        _check(c, "bytes", x, ref, dec, redo=0)
    finally:
        c[0].set_wire_format("palisade")


# ------------------------------------------------------ the single-coefficient edges ----
def _plain(c, name, api):
    """Three uniform(-1, 1) ciphertexts: the oracle's residues and decrypt, and the fast path's residues
    through `api` (no redo), which a special middle ciphertext must leave alone in its neighbours."""
    ch = c[1]
    if (name, "plain") not in _REF:
        x = np.random.default_rng(17).uniform(-1, 1, 3 * ch.S)
        _REF[(name, "plain")] = (x,) + _oracle(c, x)
    x, ref, dec = _REF[(name, "plain")]
    if (name, "fast", api) not in _REF:
        _REF[(name, "fast", api)] = _check(c, api, x, ref, dec, redo=0)
    return x, ref, dec, _REF[(name, "fast", api)]


def _middle(c, name, api, special, redo):
    """`special` as the middle ciphertext of a 3-ciphertext call."""
    ch = c[1]
    x0, ref0, _, fast = _plain(c, name, api)
    x = x0.copy()
    x[ch.S:2 * ch.S] = special
    key = (name, "middle", special.tobytes())
    if key not in _REF:
        mid, _ = _oracle(c, special, g0=1)
        ref = ref0.copy()
        ref[1] = mid[0]
        _, _, _, sk = c
        _REF[key] = (ref, O.decrypt_vector_omp(ref, sk, ch.q, ch.psi, ch.S, ch.delta, len(x), nthreads=THREADS))
    ref, dec = _REF[key]
    got = _check(c, api, x, ref, dec, redo)
    assert np.array_equal(got[0], fast[0]) and np.array_equal(got[2], fast[2])
    assert not np.array_equal(got[1], fast[1])


@pytest.mark.parametrize("api", ["device", "bytes"])
@pytest.mark.parametrize("sign", [1, -1], ids=["pos", "neg"])
@pytest.mark.parametrize("target", E.TARGETS)
@pytest.mark.parametrize("name", [PALISADE, "2^15/L4"])
def test_at_coefficient(ctx, name, target, sign, api):
    """A wrapped ciphertext (first_wrap) is compared with the oracle only: its decrypt is not close to
    x, as in PALISADE."""
    c = ctx(name)
    ch = c[1]
    t = E.at_coefficient(ch.N, ch.S, ch.delta, target)
    _middle(c, name, api, E.constant(ch.S, sign * t.c), E.REDO[target])


@pytest.mark.parametrize("api", ["device", "bytes"])
@pytest.mark.parametrize("every_slot", [False, True], ids=["one_slot", "every_slot"])
@pytest.mark.parametrize("name", [PALISADE, "2^15/L4"])
def test_huge(ctx, name, every_slot, api):
    """1e290: logApprox about 950 (ldexp(1.0, la), 2^la mod q_t, the division by 2^la)."""
    c = ctx(name)
    _middle(c, name, api, E.huge(c[1].S, every_slot), 1)


@pytest.mark.parametrize("api", ["device", "bytes"])
@pytest.mark.parametrize("name", [PALISADE, "2^15/L4"])
def test_overflow_is_refused(ctx, name, api):
    """A finite input whose scaled coefficient is infinite: refused as non-finite (the oracle returns
    -3), not counted as a redo, and the context encrypts as before afterwards."""
    c = ctx(name)
    ck, ch = c[0], c[1]
    x0, ref0, dec0, _ = _plain(c, name, api)
    x = x0.copy()
    x[ch.S:2 * ch.S] = E.overflow(ch.S, ch.delta)
    n0 = ck.encode_redo_count()
    with pytest.raises(ValueError, match="non-finite"):
        _encrypt(c, api, x)
    assert ck.encode_redo_count() == n0
    _check(c, api, x0, ref0, dec0, redo=0)
