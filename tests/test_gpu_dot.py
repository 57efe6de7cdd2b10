"""EvalInnerProduct on the MI355X: device.dot -- sum_k a_k (x) b_k with one relinearization
-- bit for bit against tests/dot_ref.py (checked for what it means by tests/test_dot_ref.py), on raw
[K][2][Ll][N] residues, every output buffer passed in filled with ones.

  chains and levels   the rings, digit shapes and levels of tests/test_gpu_f4_levels.py that change a kernel
                      or a table behind the key switch, plus the single-block ring 2^11 / L3 and 2^15 / L4,
                      on uniform and edge operands; the squared path against the general one on a copy
  the split           K = 5 under SHELFI_DOT_SLICE_CTS = 1, 2, 3 and unset, and K = 17 capped at 16 slices:
                      the slice count is what shelfi.h says and no output bit depends on it
  accumulator limits  every residue q_t - 1 (every product maximal) in ONE slice, K straddling every fold
                      interval either reading of red128's domain gives (16 products: K = 8; 256: K = 128),
                      on 60- / 52- / 53-bit towers and on the 30-bit chain; (q - 1)^2 = 1 mod q, so the
                      sums are the constants K, 2K, K
  guards              no key, K = 0, towers 0 and L + 1, out aliasing a, out overlapping b, a chain too long
                      to key-switch; a following mult is still the oracle's
  meaning             dot -> rescale -> eval_sum -> decrypt is sum x y, no worse than the per-ciphertext path
  neighbours          mult, rotate and rescale give the same bits before and after a dot in their context"""
import ctypes as C
import functools

import numpy as np
import pytest

import dot_ref as DR
import oracle as O
from conftest import set_switch
from f4_cases import _edge_batch, _full_batch, _residue_batch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

SWITCH = "SHELFI_DOT_SLICE_CTS"
DEFAULT_SLICE_CTS = 256  # shelfi_internal.h Switches::dot_slice_cts

# id: (ring, towers, scale bits, first modulus bits, alpha, [(level, K), ...])
CHAINS = {
    "n11": (1 << 11, 3, 52, 60, 2, [(3, 3)]),                             # single-block ring
    "A": (1 << 12, 7, 52, 60, 3, [(7, 3), (4, 3), (1, 3)]),
    "C": (1 << 12, 12, 52, 60, 4, [(12, 1), (12, 2), (5, 1), (5, 2)]),    # T = 16 at the top
    "D": (1 << 13, 6, 52, 60, 2, [(6, 3), (2, 3)]),
    "G": (1 << 12, 4, 30, 45, 2, [(4, 3), (3, 3), (2, 3), (1, 3)]),       # red_ok false
    "n15": (1 << 15, 4, 52, 60, 2, [(4, 3)]),
    "E": (1 << 16, 6, 52, 60, 2, [(4, 2)]),
    "F": (1 << 17, 5, 52, 60, 2, [(5, 2)]),
    "n13": (1 << 13, 3, 52, 60, 2, []),                                    # the split's context
}
CASES = [(cid, Ll, K) for cid, c in CHAINS.items() for Ll, K in c[5]]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _ones(Ll, N):
    return torch.ones((1, 2, Ll, N), dtype=torch.int64, device="cuda")


def _make(N, L, sb, fb, seed):
    c = m.CKKS("ckks", N // 2, sb, "", multDepth=L - 1, firstModBits=fb, ringDim=N, seed=seed, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    assert (inf["ring_dim"], inf["num_towers"]) == (N, L)
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    pk, sk = c.get_keys()
    return dict(c=c, inf=inf, q=q, psi=psi, sk=sk, N=N, L=L, seed=seed)


@functools.lru_cache(maxsize=None)
def chain(cid):
    """One context per chain for the whole module, with its evaluation key."""
    N, L, sb, fb, alpha = CHAINS[cid][:5]
    x = _make(N, L, sb, fb, 1400 + sum(ord(ch) for ch in cid))
    x["c"].evalMultKeyGen()
    x["evk"] = x["c"].get_eval_key()
    assert O.special_primes(N, x["q"])[1] == alpha
    x["alpha"] = alpha
    return x


def _rng(cid, Ll, salt):
    return np.random.default_rng([sum(ord(ch) for ch in cid), Ll, salt])


def _dot(x, a, b=None):
    """device.dot into a buffer of ones; b None: the squared path (the same tensor twice)."""
    ta = _dev(a)
    tb = ta if b is None else _dev(b)
    out = _ones(a.shape[2], a.shape[3])
    assert D.dot(x["c"], ta, tb, out=out) is out
    assert np.array_equal(_u64(ta), a)  # the inputs are read only
    return _u64(out)


def _ref(x, a, b):
    return DR.dot_ref(a, b, x["evk"], x["q"], x["psi"])


def _edges(x, rng, Ll, K):
    """K = 3: all q_t - 1 twice; (0, q_t - 1) against uniform; the planted c2.  K = 2: the first and the
    last of those.  K = 1: the planted c2."""
    a, b = _edge_batch(rng, x["q"], x["psi"], Ll, x["alpha"], x["N"], 3)
    keep = {1: [2], 2: [0, 2], 3: [0, 1, 2]}[K]
    return np.ascontiguousarray(a[keep]), np.ascontiguousarray(b[keep])


# ------------------------------------------------------------ chains and levels ----
@pytest.mark.parametrize("cid,Ll,K", CASES, ids=str)
def test_dot_uniform(cid, Ll, K):
    x = chain(cid)
    rng = _rng(cid, Ll, 1)
    a, b = (_residue_batch(rng, x["q"], K, Ll, x["N"]) for _ in range(2))
    got = _dot(x, a, b)
    assert got.shape == (1, 2, Ll, x["N"])
    assert np.array_equal(got, _ref(x, a, b))


@pytest.mark.parametrize("cid,Ll,K", CASES, ids=str)
def test_dot_edges(cid, Ll, K):
    x = chain(cid)
    a, b = _edges(x, _rng(cid, Ll, 2), Ll, K)
    assert np.array_equal(_dot(x, a, b), _ref(x, a, b))


@pytest.mark.parametrize("cid,Ll", [("A", 7), ("A", 4), ("G", 4), ("G", 1), ("n15", 4)], ids=str)
def test_square_is_the_general_path_on_a_copy(cid, Ll):
    x = chain(cid)
    rng = _rng(cid, Ll, 3)
    for a in (_residue_batch(rng, x["q"], 3, Ll, x["N"]), _edges(x, rng, Ll, 3)[0]):
        sq = _dot(x, a)
        assert np.array_equal(sq, _dot(x, a, a.copy()))
        assert np.array_equal(sq, _ref(x, a, a))
        ta = _dev(a)  # the same storage through another tensor object
        assert np.array_equal(_u64(D.dot(x["c"], ta, ta.view(ta.shape))), sq)


# -------------------------------------------------------------------- the split ----
def test_split_does_not_change_a_bit(monkeypatch):
    x = chain("n13")
    c, N, K = x["c"], x["N"], 5
    rng = _rng("n13", 3, 4)
    a, b = (_residue_batch(rng, x["q"], K, 3, N) for _ in range(2))
    ref = _ref(x, a, b)
    ref_sq = _ref(x, a, a)
    set_switch(monkeypatch, SWITCH, "1000")
    one = _dot(x, a, b)
    assert c.dot_slice_count() == 1
    assert np.array_equal(one, ref)
    for val, slices in (("1", 5), ("2", 3), ("3", 2), (None, min(16, -(-K // DEFAULT_SLICE_CTS)))):
        set_switch(monkeypatch, SWITCH, val)
        assert np.array_equal(_dot(x, a, b), one), val
        assert c.dot_slice_count() == slices, val
        assert np.array_equal(_dot(x, a), ref_sq), val
        assert c.dot_slice_count() == slices, val


def test_split_is_capped_at_16_slices_and_a_refusal_keeps_the_count(monkeypatch):
    x = chain("n13")
    c, N, K = x["c"], x["N"], 17
    rng = _rng("n13", 3, 5)
    a, b = (_residue_batch(rng, x["q"], K, 3, N) for _ in range(2))
    ref = _ref(x, a, b)
    set_switch(monkeypatch, SWITCH, "1")
    assert np.array_equal(_dot(x, a, b), ref)
    assert c.dot_slice_count() == 16  # 17 ciphertexts in 16 slices: one of two, fifteen of one
    assert np.array_equal(_dot(x, a), _ref(x, a, a))
    ta = _dev(a)
    with pytest.raises(ValueError, match="overlap"):
        D.dot(c, ta, ta, out=ta[3:4])
    assert c.dot_slice_count() == 16
    set_switch(monkeypatch, SWITCH, "1000")
    assert np.array_equal(_dot(x, a, b), ref)
    assert c.dot_slice_count() == 1
    with pytest.raises(ValueError):
        D.dot(c, ta[:0], ta[:0])
    assert c.dot_slice_count() == 1


# ------------------------------------------------------------ accumulator limits ----
LIMIT_K = [7, 8, 9, 15, 16, 17, 127, 128, 129, 255, 256, 257]


def _const_ref(x, Ll, K):
    """relin_ref of the three constant polynomials K, 2K, K mod q_t: what K maximal pairs sum to."""
    N = x["N"]
    c = np.empty((3, Ll, N), np.uint64)
    for t in range(Ll):
        qt = int(x["q"][t])
        c[0, t], c[1, t], c[2, t] = K % qt, 2 * K % qt, K % qt
    return DR.relin_ref(c[0], c[1], c[2], x["evk"], x["q"], x["psi"])


@pytest.mark.parametrize("K", LIMIT_K)
@pytest.mark.parametrize("cid", ["n11", "G"])
def test_maximal_products_in_one_slice(cid, K, monkeypatch):
    x = chain(cid)
    Ll, N = x["L"], x["N"]
    set_switch(monkeypatch, SWITCH, "100000")
    a = _full_batch(x["q"], K, Ll, N)
    ref = _const_ref(x, Ll, K)
    got = _dot(x, a, a.copy())
    assert x["c"].dot_slice_count() == 1
    assert np.array_equal(got, ref)
    assert np.array_equal(_dot(x, a), ref)
    assert x["c"].dot_slice_count() == 1


@pytest.mark.parametrize("cid", ["n11", "G"])
def test_maximal_a1_against_uniform_b_in_one_slice(cid, monkeypatch):
    x = chain(cid)
    Ll, N, K = x["L"], x["N"], 17
    set_switch(monkeypatch, SWITCH, "100000")
    rng = _rng(cid, Ll, 6)
    a, b = (_residue_batch(rng, x["q"], K, Ll, N) for _ in range(2))
    a[:, 1] = _full_batch(x["q"], K, Ll, N)[:, 1]
    assert np.array_equal(_dot(x, a, b), _ref(x, a, b))
    assert x["c"].dot_slice_count() == 1


# ----------------------------------------------------------------------- guards ----
def _mult_is_the_oracles(x, a, b):
    got = _u64(D.mult(x["c"], _dev(a), _dev(b)))
    assert np.array_equal(got, O.eval_mult(a, b, x["evk"], x["q"], x["psi"]))


def test_guards():
    x = chain("D")
    c, q, N, L = x["c"], x["q"], x["N"], x["L"]
    lib = _lib.load()
    rng = _rng("D", 4, 7)
    a, b = (_residue_batch(rng, q, 3, 4, N) for _ in range(2))
    ta, tb = _dev(a), _dev(b)
    out = _ones(4, N)
    good = _dot(x, a, b)
    count = c.dot_slice_count()

    def raw(pa, pb, K, towers, po):
        return lib.shelfi_dev_dot(c._ctx, C.c_void_p(pa), C.c_void_p(pb), K, towers, C.c_void_p(po), None)

    pa, pb, po = ta.data_ptr(), tb.data_ptr(), out.data_ptr()
    ctb = 2 * 4 * N * 8
    # (buffers as large as the refused tower count would need: the call under test stays inside them)
    wide = [torch.zeros((3, 2, L + 1, N), dtype=torch.int64, device="cuda") for _ in range(3)]
    wa, wb, wo = (t.data_ptr() for t in wide)
    refused = [
        lambda: raw(pa, pb, 0, 4, po),                    # K = 0
        lambda: raw(pa, pb, 3, 0, po),                    # towers 0
        lambda: raw(wa, wb, 3, L + 1, wo),                # towers L + 1
        lambda: raw(None, pb, 3, 4, po),                  # NULL buffers
        lambda: raw(pa, None, 3, 4, po),
        lambda: raw(pa, pb, 3, 4, None),
        lambda: raw(pa, pb, 3, 4, pa),                    # out aliasing a
        lambda: raw(pa, pb, 3, 4, pb + 2 * ctb),          # out overlapping b by one ciphertext
        lambda: raw(pa, pb, 3, 4, pb + ctb + ctb // 2),   # ... at a shift inside b
        lambda: raw(pa, pa, 3, 4, pa + ctb),              # the squared path's one input
    ]
    for i, call in enumerate(refused):
        assert call() == _lib.SHELFI_ERR_ARG, i
        assert c.dot_slice_count() == count, i
        assert torch.equal(out, _ones(4, N)), i
        _mult_is_the_oracles(x, a[:1], b[:1])
    # the same through device.dot
    for call in (lambda: D.dot(c, ta[:0], tb[:0]),
                 lambda: D.dot(c, ta[:1], tb[:1], out=ta[:1]),
                 lambda: D.dot(c, ta, tb, out=tb[2:3]),
                 lambda: D.dot(c, ta, tb[:2]),
                 lambda: D.dot(c, ta, tb, out=_ones(3, N)),
                 lambda: D.dot(c, ta[:, :, :0].contiguous(), tb[:, :, :0].contiguous()),
                 lambda: D.dot(c, torch.zeros((3, 2, L + 1, N), dtype=torch.int64, device="cuda"),
                               torch.zeros((3, 2, L + 1, N), dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            call()
        assert c.dot_slice_count() == count
    assert np.array_equal(_u64(ta), a) and np.array_equal(_u64(tb), b)
    _mult_is_the_oracles(x, a, b)
    assert np.array_equal(_dot(x, a, b), good)


def test_no_evaluation_key_is_a_state_error():
    x = _make(1 << 11, 3, 52, 60, 1451)
    c, q, N = x["c"], x["q"], x["N"]
    a = _residue_batch(np.random.default_rng(8), q, 2, 3, N)
    out = _ones(3, N)
    with pytest.raises(RuntimeError, match="evaluation key") as e:
        D.dot(c, _dev(a), _dev(a), out=out)
    assert e.value.code == _lib.SHELFI_ERR_STATE
    assert torch.equal(out, _ones(3, N)) and c.dot_slice_count() == 0
    c.evalMultKeyGen()
    x["evk"] = c.get_eval_key()
    _mult_is_the_oracles(x, a, a[::-1].copy())
    assert np.array_equal(_u64(D.dot(c, _dev(a), _dev(a), out=out)), _ref(x, a, a))


def test_chain_too_long_is_refused_by_name():
    """tests/f4_cases.py's 13-tower chain: 5 special primes, 18 towers; no key can exist, and the call
    says why rather than asking for one."""
    x = _make(1 << 12, 13, 52, 60, 1413)
    c, q, N = x["c"], x["q"], x["N"]
    assert len(O.special_primes(N, q)[2]) == 5
    a = _dev(_residue_batch(np.random.default_rng(9), q, 2, 13, N))
    for call in (lambda: D.dot(c, a, a), lambda: D.dot(c, a[:, :, :2].contiguous(), a[:, :, :2].contiguous())):
        with pytest.raises(ValueError, match="<= 16"):
            call()
    assert c.dot_slice_count() == 0 and not c.eval_key_info()["has_key"]


# ---------------------------------------------------------------------- meaning ----
def test_dot_rescale_eval_sum_decrypts_to_the_inner_product():
    """2^12 / L3, K = 4 ciphertexts of 2048 slots: every slot of the one result holds sum x y over all
    8192 values; the per-ciphertext path (K mults, K ModReduces, the adds) reaches the same number with K
    key-switch errors where dot has one."""
    x = _make(1 << 12, 3, 52, 60, 1461)
    c, q, N, inf = x["c"], x["q"], x["N"], x["inf"]
    c.evalMultKeyGen()
    c.evalSumKeyGen()
    S, K = inf["batch"], 4
    rng = np.random.default_rng(10)
    xs, ys = rng.uniform(-1, 1, K * S), rng.uniform(-1, 1, K * S)
    u = D.encrypt(c, torch.tensor(xs, dtype=torch.float64, device="cuda"))
    v = D.encrypt(c, torch.tensor(ys, dtype=torch.float64, device="cuda"))
    assert u.shape == (K, 2, 3, N)
    scale = inf["delta"] * inf["delta"] / float(q[2])
    exp = float(np.dot(xs, ys))

    tot = D.eval_sum(c, D.rescale(c, D.dot(c, u, v)), S)
    assert tot.shape == (1, 2, 2, N)
    dec = D.decrypt(c, tot, S, scale).cpu().numpy()
    err_dot = float(np.abs(dec - exp).max())

    prod = D.rescale(c, D.mult(c, u, v))
    acc = prod[0:1].clone()
    for k in range(1, K):
        D.add(c, acc, prod[k:k + 1].contiguous(), out=acc)
    dec_p = D.decrypt(c, D.eval_sum(c, acc, S), S, scale).cpu().numpy()
    err_par = float(np.abs(dec_p - exp).max())
    print("sum x y = %.6f: dot path error %.3g, per-ciphertext path error %.3g" % (exp, err_dot, err_par))
    assert err_dot < 1e-6 and err_par < 1e-6
    assert err_dot <= 4 * err_par

    sq = D.decrypt(c, D.eval_sum(c, D.rescale(c, D.dot(c, u, u)), S), S, scale).cpu().numpy()
    assert float(np.abs(sq - np.dot(xs, xs)).max()) < 1e-6


# ------------------------------------------------------------------- neighbours ----
def test_neighbours_give_the_same_bits_around_a_dot():
    x = chain("n13")
    c, q, N = x["c"], x["q"], x["N"]
    c.rotationKeyGen([3])
    rng = _rng("n13", 3, 11)
    a, b = (_dev(_residue_batch(rng, q, 2, 3, N)) for _ in range(2))

    def neighbours():
        return D.mult(c, a, b), D.rotate(c, a, 3), D.rescale(c, b)

    before = neighbours()
    big = _dev(_residue_batch(rng, q, 9, 3, N))  # a larger scratch than the neighbours took
    D.dot(c, big, big)
    D.dot(c, big, big.flip(0).contiguous())
    for u, v in zip(before, neighbours()):
        assert torch.equal(u, v)
