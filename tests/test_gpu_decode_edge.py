"""Decrypt at the edge of its value range on chains the fast path decodes whole (at or below 2^130:
multDepth = 1, the reference's fixed setting, ckks.cpp:26; one or two towers at a lower level).

There the fast CRT's binary32 quotient k can be off by one for a coefficient within ~Q 2^-19 of
+-(Q-1)/2, which gives X -+ Q -- still inside (-2^127, 2^127), so the 128-bit range flag cannot see it.
crt_value's EDGE variant flags every |X'| >= (Q-1)/2 - floor(Q 2^-16) and the call is redone through the
exact CRT (tests/test_decode_towers.py holds the bit-level model to the same rule).

The ciphertexts are built, not encrypted: c1 = 0 and c0 = the per-tower forward NTT of chosen integer
coefficients, so c0 + c1 s decrypts to exactly those integers whatever the key is.  With batch = N/2
every coefficient is a slot part (re_i = c[i], im_i = c[N/2 + i]).  Per case one call of two ciphertexts:
a mixed one (half the coefficients ordinary, |X| < Q/4; half X = +-((Q-1)/2 - d), d uniform in
[0, Q 2^-19) and d in {0, 1, 2}) and an ordinary-only one; then the ordinary one alone, which must stay
on the fast path (redo count unchanged).

Contexts and the kernel each takes (launch_decrypt): multDepth = 1 at 2^13 (ntt_inv_cols_crt<2, 5>
fused), 2^11 (one NTT block, logR = 0: the stand-alone crt_decode_kernel), and the 1- and 2-tower
slices of a 2^15 / L4 context through device.decrypt (level tables, ntt_inv_cols_crt<4, 5>).

Tolerances: bit-equal to the oracle's decrypt (multi-word centring, Horner conversion, the same FFT
order); within 2^-30 Q/scale of an independent reference (Python-integer coefficients -> double ->
O.fft_special): a coefficient off by Q moves some slot by more than Q / (2 scale), the double FFT's
rounding at these sizes is below 2^-36 Q/scale."""
import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402


def _make(tmp_path_factory, name, batch, depth, seed, **kw):
    d = str(tmp_path_factory.mktemp(name)) + os.sep
    ck = m.CKKS("ckks", batch, 52, d, multDepth=depth, seed=seed, decodeNoise=False, **kw)
    assert ck.genCryptoContextAndKeyGen() == 1
    return ck


@pytest.fixture(scope="module")
def ctx13(tmp_path_factory):
    return _make(tmp_path_factory, "edge13", 4096, 1, 21)  # the reference default: 2^13, L2


@pytest.fixture(scope="module")
def ctx11(tmp_path_factory):
    return _make(tmp_path_factory, "edge11", 1024, 1, 22, ringDim=2048)  # one NTT block: no fused CRT


@pytest.fixture(scope="module")
def ctx15(tmp_path_factory):
    return _make(tmp_path_factory, "edge15", 16384, 3, 23)  # 2^15, L4: sliced to 1 and 2 towers


CASES = {  # name: (context fixture, ring, towers decoded (0 = the chain), APIs)
    "2^13/L2": ("ctx13", 1 << 13, 0),
    "2^11/L2": ("ctx11", 1 << 11, 0),
    "2^15/L4 one tower": ("ctx15", 1 << 15, 1),
    "2^15/L4 two towers": ("ctx15", 1 << 15, 2),
}
_built = {}


def _rand_below(rng, bound):
    return int.from_bytes(rng.bytes(24), "little") % bound


def _coeffs(Q, N, rng, mixed):
    """N integer coefficients: ordinary ones, |X| < Q/4; mixed: a random half of the positions at the
    edge instead, X = +-((Q-1)/2 - d) with d in {0, 1, 2} (both signs) and d uniform in [0, Q 2^-19)."""
    X = [_rand_below(rng, Q // 4) * (1 if rng.integers(2) else -1) for _ in range(N)]
    if mixed:
        half = (Q - 1) // 2
        pos = rng.permutation(N)[:N // 2]
        for n, p in enumerate(pos):
            d = n // 2 if n < 6 else _rand_below(rng, Q >> 19)
            X[int(p)] = (half - d) * (1 if n % 2 else -1)
    return X


def _case(name, ck):
    """The case's two ciphertexts [2][2][T][N], their integer coefficients, and both references --
    computed once and shared by the APIs."""
    if name in _built:
        return _built[name]
    _, ring, T = CASES[name]
    inf = ck.info()
    N, S, delta = inf["ring_dim"], inf["batch"], inf["delta"]
    assert N == ring and S == N // 2
    T = T or inf["num_towers"]
    q = [int(v) for v in inf["moduli"][:T]]
    psi = [int(v) for v in inf["roots"][:T]]
    assert sum(v.bit_length() - 1 for v in q) <= 130  # decoded whole (decode_towers)
    Q = 1
    for v in q:
        Q *= v
    rng = np.random.default_rng(ring + T)
    Xs = [_coeffs(Q, N, rng, True), _coeffs(Q, N, rng, False)]
    res = np.zeros((2, 2, T, N), np.uint64)
    for k, X in enumerate(Xs):
        for t in range(T):
            res[k, 0, t] = O.ntt_fwd(np.array([x % q[t] for x in X], np.uint64), q[t], psi[t])
    _, sk = ck.get_keys()
    sk = np.ascontiguousarray(sk[:T])
    qa, pa = np.array(q, np.uint64), np.array(psi, np.uint64)
    indep = np.zeros(2 * S)
    for k, X in enumerate(Xs):
        fx = np.array([float(x) for x in X]) / delta
        # the layout: the oracle reads the built ciphertext back as these integers (its Horner
        # conversion of a two-word |X| may differ from float(X)'s single rounding by one ulp)
        re, im = O.decrypt_coeffs(res[k], sk, qa, pa, S, delta)
        assert np.all(np.abs(np.concatenate([re, im]) - fx) <= 2.0 ** -52 * np.abs(fx))
        indep[k * S:(k + 1) * S] = O.fft_special(fx[:S] + 1j * fx[S:]).real
    ref = O.decrypt_vector(res, sk, qa, pa, S, delta, 2 * S)
    assert np.abs(ref - indep).max() <= 2.0 ** -30 * float(Q) / delta  # the two references agree
    _built[name] = (res, ref, indep, float(Q) / delta, S, delta)
    return _built[name]


def _decrypt(ck, api, res, n, delta):
    if api == "bytes":
        return np.asarray(ck.decrypt(m.blob_pack(ck, res), n))
    return D.decrypt(ck, torch.from_numpy(res.view(np.int64)).cuda(), n, delta).cpu().numpy()


@pytest.mark.parametrize("name,api", [("2^13/L2", "bytes"), ("2^13/L2", "device"), ("2^11/L2", "bytes"),
                                      ("2^11/L2", "device"), ("2^15/L4 one tower", "device"),
                                      ("2^15/L4 two towers", "device")])
def test_short_chain_near_half_q(name, api, request):
    ck = request.getfixturevalue(CASES[name][0])
    res, ref, indep, qs, S, delta = _case(name, ck)
    n0 = ck.decode_redo_count()
    out = _decrypt(ck, api, res, 2 * S, delta)  # the mixed ciphertext and the ordinary one
    n1 = ck.decode_redo_count()
    err = np.abs(out - indep).max()
    print("%s %s: max |out - indep| = %.3g Q/scale, %d of %d values differ from the oracle, redo %d"
          % (name, api, err / qs, int((out != ref).sum()), out.size, n1 - n0))
    assert err <= 2.0 ** -30 * qs
    assert np.array_equal(out, ref)
    assert n1 - n0 == 1  # the edge coefficients sent the call to the exact pass
    out = _decrypt(ck, api, res[1:], S, delta)  # ordinary values alone stay on the fast path
    assert np.array_equal(out, ref[S:])
    assert ck.decode_redo_count() - n1 == 0
