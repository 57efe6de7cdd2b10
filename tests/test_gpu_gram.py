"""The Gram matrix of encrypted batches on the MI355X: device.gram -- every pairwise
EvalInnerProduct of C batches, one batched relinearization -- bit for bit against tests/gram_ref.py (checked for
what it means by tests/test_gram_ref.py), on raw [K][2][Ll][N] residues, every output buffer passed in filled
with ones.

  tile geometry       C = 1..7 and 16 at 2^11 / L3: every full, diagonal and ragged tile of the 2 x 2 tiling,
                      one reference shared; C = 5 as separate tensors, as views of a stack and as the stack
  against dot         every entry is device.dot of its pair, the diagonal the squared path; one tensor at two
                      indices gives equal rows and the squared result between them
  chains and levels   the rings, digit shapes and levels of tests/test_gpu_dot.py, C = 3, K = 2
  fold edges          every residue q_t - 1 (every product maximal) in ONE slice, K straddling the 128-ciphertext
                      fold of a 60-bit tower and twice it, on 60- / 52- / 53-bit and on 45- / 31- / 30-bit
                      towers: (q - 1)^2 = 1 mod q, so every pair's sums are the constants K, 2K, K
  slices, chains      no output bit depends on SHELFI_GRAM_SLICE_CTS or on SHELFI_EVAL_CHUNK_MIB, and both
                      counters say what include/shelfi.h says
  guards              every refusal of shelfi_dev_gram; a following mult is still the oracle's
  meaning             gram -> rescale -> eval_sum -> decrypt is <x_i, x_j>; gram_sq_distances is ||x_i - x_j||^2
  neighbours          mult, rotate, rescale and dot give the same bits before and after a gram"""
import ctypes as C
import functools

import numpy as np
import pytest

import dot_ref as DR
import gram_ref as GR
import oracle as O
from conftest import set_switch
from f4_cases import _edge_batch, _full_batch, _residue_batch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

SLICE = "SHELFI_GRAM_SLICE_CTS"
CHUNK = "SHELFI_EVAL_CHUNK_MIB"
DEFAULT_SLICE_CTS = 256  # shelfi_internal.h Switches::gram_slice_cts
FILL_GROUPS = 1024       # shelfi_internal.h kGramFillGroups
TILE = 2                 # shelfi_internal.h kGramTile

# id: (ring, towers, scale bits, first modulus bits, [level, ...])
CHAINS = {
    "n11": (1 << 11, 3, 52, 60, []),                 # single-block ring: geometry and the 60-bit fold
    "g11": (1 << 11, 3, 30, 45, []),                 # 45- / 31- / 30-bit towers: red_ok false, no fold in reach
    "A": (1 << 12, 7, 52, 60, [7, 4, 1]),
    "C": (1 << 12, 12, 52, 60, [12, 5]),             # T = 16 at the top
    "D": (1 << 13, 6, 52, 60, [6]),
    "G": (1 << 12, 4, 30, 45, [4, 3, 2, 1]),         # red_ok false
    "n15": (1 << 15, 4, 52, 60, [4]),
    "E": (1 << 16, 6, 52, 60, [4]),
    "F": (1 << 17, 5, 52, 60, [5]),
    "n13": (1 << 13, 3, 52, 60, []),                 # slices, chains, neighbours
}
CASES = [(cid, Ll) for cid, c in CHAINS.items() for Ll in c[4]]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _ones(P, Ll, N):
    return torch.ones((P, 2, Ll, N), dtype=torch.int64, device="cuda")


def _make(N, L, sb, fb, seed):
    c = m.CKKS("ckks", N // 2, sb, "", multDepth=L - 1, firstModBits=fb, ringDim=N, seed=seed, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    assert (inf["ring_dim"], inf["num_towers"]) == (N, L)
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    return dict(c=c, inf=inf, q=q, psi=psi, N=N, L=L, seed=seed)


@functools.lru_cache(maxsize=None)
def chain(cid):
    """One context per chain for the whole module, with its evaluation key."""
    N, L, sb, fb = CHAINS[cid][:4]
    x = _make(N, L, sb, fb, 1500 + sum(ord(ch) for ch in cid))
    x["c"].evalMultKeyGen()
    x["evk"] = x["c"].get_eval_key()
    x["alpha"] = O.special_primes(N, x["q"])[1]
    return x


def _rng(cid, Ll, salt):
    return np.random.default_rng([sum(ord(ch) for ch in cid), Ll, salt])


def _gram(x, us, how="separate"):
    """device.gram into a buffer of ones.  how: the batches as separate allocations, as views of one stacked
    tensor, or the stacked tensor itself."""
    n, (K, _, Ll, N) = len(us), us[0].shape
    if how == "separate":
        ts = [_dev(u) for u in us]
        arg = ts
    else:
        stack = _dev(np.stack(us))
        ts = [stack[i] for i in range(n)]
        arg = ts if how == "views" else stack
    out = _ones(n * (n + 1) // 2, Ll, N)
    assert D.gram(x["c"], arg, out=out) is out
    for t, u in zip(ts, us):
        assert np.array_equal(_u64(t), u)  # the inputs are read only
    return _u64(out)


def _ref(x, us):
    return GR.gram_ref(us, x["evk"], x["q"], x["psi"])


# ---------------------------------------------------------------- tile geometry ----
GEOMETRY_C = [1, 2, 3, 4, 5, 6, 7, 16]


@functools.lru_cache(maxsize=None)
def _geometry():
    """16 uniform batches of K = 3 at 2^11 / L3 and their Gram reference; the reference over the first C of
    them is its entries (i, j), i <= j < C."""
    x = chain("n11")
    rng = _rng("n11", 3, 1)
    us = [_residue_batch(rng, x["q"], 3, 3, x["N"]) for _ in range(16)]
    ref = _ref(x, us)
    ref.setflags(write=False)
    return us, ref


def _geometry_ref(n):
    us, ref = _geometry()
    return us[:n], ref[[GR.pair_index(i, j, 16) for i, j in GR.pairs(n)]]


@pytest.mark.parametrize("n", GEOMETRY_C)
def test_every_tile_shape(n):
    x = chain("n11")
    us, ref = _geometry_ref(n)
    got = _gram(x, us)
    assert got.shape == (n * (n + 1) // 2, 2, 3, x["N"])
    assert np.array_equal(got, ref)
    assert x["c"].eval_chunk_count() == 1
    assert D.gram_pairs(n) == GR.pairs(n) and _lib.load().shelfi_gram_pairs(n) == len(GR.pairs(n))


@pytest.mark.parametrize("how", ["separate", "views", "stacked"])
def test_batches_given_three_ways(how):
    us, ref = _geometry_ref(5)
    assert np.array_equal(_gram(chain("n11"), us, how), ref)


# ----------------------------------------------------------------- against dot ----
def test_every_entry_is_dot_of_its_pair():
    x = chain("n11")
    c = x["c"]
    us, ref = _geometry_ref(5)
    got = _gram(x, us)
    ts = [_dev(u) for u in us]
    for p, (i, j) in enumerate(GR.pairs(5)):
        assert np.array_equal(_u64(D.dot(c, ts[i], ts[j])), got[p:p + 1]), (i, j)  # (i == j: the squared path)
    # one tensor at indices 1 and 3: equal rows, and the squared result between them
    rep = [ts[0], ts[1], ts[2], ts[1], ts[4]]
    out = _ones(15, 3, x["N"])
    g = _u64(D.gram(c, rep, out=out))
    at = {ij: p for p, ij in enumerate(GR.pairs(5))}
    sq = _u64(D.dot(c, ts[1], ts[1]))
    for p in (at[1, 1], at[1, 3], at[3, 3]):
        assert np.array_equal(g[p:p + 1], sq)
    for a, b in ((at[0, 1], at[0, 3]), (at[1, 2], at[2, 3]), (at[1, 4], at[3, 4])):
        assert np.array_equal(g[a], g[b])
    keep = [p for p, (i, j) in enumerate(GR.pairs(5)) if 3 not in (i, j)]
    assert np.array_equal(g[keep], got[keep])


# ----------------------------------------------------------- chains and levels ----
@pytest.mark.parametrize("cid,Ll", CASES, ids=str)
def test_chains_and_levels(cid, Ll):
    x = chain(cid)
    rng = _rng(cid, Ll, 2)
    us = [_residue_batch(rng, x["q"], 2, Ll, x["N"]) for _ in range(3)]
    got = _gram(x, us)
    assert got.shape == (6, 2, Ll, x["N"])
    assert np.array_equal(got, _ref(x, us))


# ------------------------------------------------------------------ fold edges ----
@functools.lru_cache(maxsize=None)
def _const_ref(cid, K):
    """relin_ref of the three constant polynomials K, 2K, K mod q_t: what K maximal products sum to, in every
    pair, on and off the diagonal."""
    x = chain(cid)
    Ll, N = x["L"], x["N"]
    c = np.empty((3, Ll, N), np.uint64)
    for t in range(Ll):
        qt = int(x["q"][t])
        c[0, t], c[1, t], c[2, t] = K % qt, 2 * K % qt, K % qt
    return DR.relin_ref(c[0], c[1], c[2], x["evk"], x["q"], x["psi"])


@pytest.mark.parametrize("K", [127, 128, 129, 257])
@pytest.mark.parametrize("cid", ["n11", "g11"])
def test_maximal_products_in_one_slice(cid, K, monkeypatch):
    x = chain(cid)
    Ll, N = x["L"], x["N"]
    set_switch(monkeypatch, SLICE, "100000")
    full = _full_batch(x["q"], K, Ll, N)
    stack = _dev(np.stack([full] * 3))
    out = _ones(6, Ll, N)
    got = _u64(D.gram(x["c"], stack, out=out))
    assert x["c"].gram_slice_count() == 1
    ref = _const_ref(cid, K)
    for p in range(6):
        assert np.array_equal(got[p:p + 1], ref), GR.pairs(3)[p]


@pytest.mark.parametrize("cid", ["n11", "g11"])
def test_one_maximal_learner_against_uniform_ones(cid, monkeypatch):
    x = chain(cid)
    Ll, N, K = x["L"], x["N"], 17
    set_switch(monkeypatch, SLICE, "100000")
    rng = _rng(cid, Ll, 3)
    us = [_residue_batch(rng, x["q"], K, Ll, N), _full_batch(x["q"], K, Ll, N), _residue_batch(rng, x["q"], K, Ll, N)]
    assert np.array_equal(_gram(x, us), _ref(x, us))
    assert x["c"].gram_slice_count() == 1


# ---------------------------------------------------------------------- slices ----
def _slices(n, K, towers, N, cts):
    """include/shelfi.h: min(16, ceil(K / cts), ceil(1024 / workgroups a slice))."""
    tiles = -(-n // TILE) * (-(-n // TILE) + 1) // 2
    groups = tiles * towers * max(1, N // 512)
    return min(16, -(-K // cts), -(-FILL_GROUPS // groups))


def test_slices_do_not_change_a_bit(monkeypatch):
    x = chain("n13")
    c, N, K = x["c"], x["N"], 5
    rng = _rng("n13", 3, 4)
    us = [_residue_batch(rng, x["q"], K, 3, N) for _ in range(2)]
    ref = _ref(x, us)
    set_switch(monkeypatch, SLICE, "1000")
    one = _gram(x, us)
    assert c.gram_slice_count() == 1
    assert np.array_equal(one, ref)
    for val, slices in (("1", 5), ("2", 3), ("3", 2), (None, 1)):
        set_switch(monkeypatch, SLICE, val)
        assert np.array_equal(_gram(x, us), one), val
        assert c.gram_slice_count() == slices == _slices(2, K, 3, N, int(val or DEFAULT_SLICE_CTS)), val


def test_slices_are_capped_at_16_and_a_refusal_keeps_the_count(monkeypatch):
    x = chain("n13")
    c, N, K = x["c"], x["N"], 17
    rng = _rng("n13", 3, 5)
    us = [_residue_batch(rng, x["q"], K, 3, N) for _ in range(2)]
    set_switch(monkeypatch, SLICE, "1")
    assert np.array_equal(_gram(x, us), _ref(x, us))
    assert c.gram_slice_count() == 16 == _slices(2, K, 3, N, 1)  # 17 ciphertexts: one slice of two, fifteen of one
    ts = [_dev(u) for u in us]
    with pytest.raises(ValueError, match="overlap"):
        D.gram(c, ts, out=ts[0][3:6])
    assert c.gram_slice_count() == 16


# --------------------------------------------------------------------- chunking ----
def test_chains_of_tiles_do_not_change_a_bit(monkeypatch):
    """2^13 / 3 towers, C = 4: 3 tiles, 10 pairs; a tile's scratch is 9.5 MiB (4 pairs: 29 + 9 polynomials of
    2^13 words each), so budgets of 1 and 10 MiB run one tile a chain and 20 MiB two tiles, then one."""
    x = chain("n13")
    c, N = x["c"], x["N"]
    rng = _rng("n13", 3, 6)
    us = [_residue_batch(rng, x["q"], 2, 3, N) for _ in range(4)]
    whole = _gram(x, us)
    assert c.eval_chunk_count() == 1
    assert np.array_equal(whole, _ref(x, us))
    for mib, chains in (("1", 3), ("10", 3), ("20", 2)):
        set_switch(monkeypatch, CHUNK, mib)
        assert np.array_equal(_gram(x, us, "stacked"), whole), mib
        assert c.eval_chunk_count() == chains, mib
    set_switch(monkeypatch, CHUNK, "1")
    us5 = us + [_residue_batch(rng, x["q"], 2, 3, N)]  # an odd C: ragged tiles in chains of their own
    got = _gram(x, us5)
    assert c.eval_chunk_count() == 6
    set_switch(monkeypatch, CHUNK, None)
    assert np.array_equal(_gram(x, us5), got) and c.eval_chunk_count() == 1
    assert np.array_equal(got[[GR.pair_index(i, j, 5) for i, j in GR.pairs(4)]], whole)


# ----------------------------------------------------------------------- guards ----
def _mult_is_the_oracles(x, a, b):
    got = _u64(D.mult(x["c"], _dev(a), _dev(b)))
    assert np.array_equal(got, O.eval_mult(a, b, x["evk"], x["q"], x["psi"]))


def test_guards():
    x = chain("D")
    c, q, N, L = x["c"], x["q"], x["N"], x["L"]
    lib = _lib.load()
    rng = _rng("D", 4, 7)
    n, K, Ll, P = 3, 3, 4, 6
    us = [_residue_batch(rng, q, K, Ll, N) for _ in range(n)]
    good = _gram(x, us)
    counts = (c.gram_slice_count(), c.eval_chunk_count())
    # the inputs in one arena with room for an output behind them: an overlapping call stays inside it
    arena = torch.zeros((n * K + P, 2, Ll, N), dtype=torch.int64, device="cuda")
    for i, u in enumerate(us):
        arena[i * K:(i + 1) * K] = _dev(u)
    before = arena.clone()
    ctb = 2 * Ll * N * 8
    base = arena.data_ptr()
    ptr = [base + i * K * ctb for i in range(n)]
    out = _ones(P, Ll, N)
    po = out.data_ptr()
    # (buffers as large as the refused shapes would need: the call under test stays inside them)
    wide = torch.zeros((n * K + P, 2, L + 1, N), dtype=torch.int64, device="cuda")
    wptr = [wide.data_ptr() + i * K * 2 * (L + 1) * N * 8 for i in range(n)]
    many = torch.zeros((33, 1, 2, Ll, N), dtype=torch.int64, device="cuda")
    mout = torch.ones((33 * 34 // 2, 2, Ll, N), dtype=torch.int64, device="cuda")

    def raw(ptrs, nb, Kc, towers, o):
        arr = None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)
        return lib.shelfi_dev_gram(c._ctx, arr, nb, Kc, towers, C.c_void_p(o), None)

    def last():
        return lib.shelfi_last_error().decode()

    assert raw(ptr, 0, K, Ll, po) == _lib.SHELFI_ERR_ARG and "1..32" in last()       # C = 0 and C = 33, by name
    assert raw([many[i].data_ptr() for i in range(33)], 33, 1, Ll, mout.data_ptr()) == _lib.SHELFI_ERR_ARG
    assert "1..32" in last() and bool((mout == 1).all())
    del mout
    refused = [
        lambda: raw(ptr, 0, K, Ll, po),                                      # C = 0
        lambda: raw(ptr, n, 0, Ll, po),                                      # K = 0
        lambda: raw(ptr, n, K, 0, po),                                       # towers 0
        lambda: raw(wptr, n, K, L + 1, wide.data_ptr() + n * K * 2 * (L + 1) * N * 8),  # towers L + 1
        lambda: raw(None, n, K, Ll, po),                                     # NULL pointers
        lambda: raw([ptr[0], None, ptr[2]], n, K, Ll, po),
        lambda: raw(ptr, n, K, Ll, None),
        lambda: raw(ptr, n, K, Ll, ptr[0]),                                  # out aliasing the first input
        lambda: raw(ptr, n, K, Ll, ptr[1]),                                  # ... an inner one
        lambda: raw(ptr, n, K, Ll, ptr[2] + 2 * ctb),                        # out overlapping the last input by one ciphertext
        lambda: raw(ptr, n, K, Ll, ptr[2] + ctb + ctb // 2),                 # ... at a shift inside it
        lambda: raw([ptr[1], ptr[2], ptr[2]], n, K, Ll, ptr[0] + ctb),       # out's tail reaching into an input given twice
    ]
    for i, call in enumerate(refused):
        assert call() == _lib.SHELFI_ERR_ARG, i
        assert (c.gram_slice_count(), c.eval_chunk_count()) == counts, i
        assert torch.equal(out, _ones(P, Ll, N)) and torch.equal(arena, before), i
        assert not bool(wide.any()), i
        _mult_is_the_oracles(x, us[0][:1], us[1][:1])
        counts = (counts[0], c.eval_chunk_count())  # (the mult's own chain count)
    # the same through device.gram
    ts = [arena[i * K:(i + 1) * K] for i in range(n)]
    for call in (lambda: D.gram(c, []),
                 lambda: D.gram(c, [many[i] for i in range(33)]),
                 lambda: D.gram(c, [t[:0] for t in ts]),
                 lambda: D.gram(c, ts, out=arena[:P]),
                 lambda: D.gram(c, ts, out=arena[n * K - 1:n * K - 1 + P]),
                 lambda: D.gram(c, [ts[0], ts[1][:2]]),
                 lambda: D.gram(c, ts, out=_ones(P - 1, Ll, N)),
                 lambda: D.gram(c, ts, out=_ones(P, Ll - 1, N)),
                 lambda: D.gram(c, [t[:, :, :0].contiguous() for t in ts]),
                 lambda: D.gram(c, arena[:n * K].view(n, K, 2, Ll, N)[:, :, :1]),
                 lambda: D.gram(c, [wide[:K], wide[K:2 * K]])):
        with pytest.raises(ValueError):
            call()
        assert c.gram_slice_count() == counts[0]
    assert torch.equal(arena, before)
    _mult_is_the_oracles(x, us[0], us[1])
    assert np.array_equal(_u64(D.gram(c, ts, out=arena[n * K:])), good)


def test_no_evaluation_key_is_a_state_error():
    x = _make(1 << 11, 3, 52, 60, 1551)
    c, q, N = x["c"], x["q"], x["N"]
    us = [_residue_batch(np.random.default_rng(8), q, 2, 3, N) for _ in range(2)]
    out = _ones(3, 3, N)
    with pytest.raises(RuntimeError, match="evaluation key") as e:
        D.gram(c, [_dev(u) for u in us], out=out)
    assert e.value.code == _lib.SHELFI_ERR_STATE
    assert torch.equal(out, _ones(3, 3, N)) and c.gram_slice_count() == 0 and c.eval_chunk_count() == 0
    c.evalMultKeyGen()
    x["evk"] = c.get_eval_key()
    _mult_is_the_oracles(x, us[0], us[1])
    assert np.array_equal(_u64(D.gram(c, [_dev(u) for u in us], out=out)), _ref(x, us))


def test_chain_too_long_is_refused_by_name():
    """tests/f4_cases.py's 13-tower chain: 5 special primes, 18 towers; no key can exist, and the call says why
    rather than asking for one."""
    x = _make(1 << 12, 13, 52, 60, 1513)
    c, q, N = x["c"], x["q"], x["N"]
    assert len(O.special_primes(N, q)[2]) == 5
    a = _dev(_residue_batch(np.random.default_rng(9), q, 2, 13, N))
    for call in (lambda: D.gram(c, [a, a]), lambda: D.gram(c, [a[:, :, :2].contiguous()] * 2)):
        with pytest.raises(ValueError, match="<= 16"):
            call()
    assert c.gram_slice_count() == 0 and not c.eval_key_info()["has_key"]


# ---------------------------------------------------------------------- meaning ----
def test_gram_rescale_eval_sum_decrypts_to_the_inner_products():
    """2^12 / L3, C = 4 learners of K = 2 ciphertexts of 2048 slots: after ModReduce and EvalSum over the
    slots, slot 0 of pair p holds <x_i, x_j> over all 4096 values (test_gpu_dot.py's end-to-end bound), and
    gram_sq_distances -- four entries a distance -- holds ||x_i - x_j||^2 within four times that.  Measured:
    2.0e-10 and 3.9e-10."""
    x = _make(1 << 12, 3, 52, 60, 1561)
    c, q, N, inf = x["c"], x["q"], x["N"], x["inf"]
    c.evalMultKeyGen()
    c.evalSumKeyGen()
    S, K, n = inf["batch"], 2, 4
    xs = np.random.default_rng(10).uniform(-1, 1, (n, K * S))
    us = [D.encrypt(c, torch.tensor(v, dtype=torch.float64, device="cuda")) for v in xs]
    assert us[0].shape == (K, 2, 3, N)
    scale = inf["delta"] * inf["delta"] / float(q[2])
    G = D.gram(c, us)
    P = len(GR.pairs(n))
    assert G.shape == (P, 2, 3, N)

    tot = D.eval_sum(c, D.rescale(c, G), S)
    dec = D.decrypt(c, tot, P * S, scale).cpu().numpy().reshape(P, S)
    exp = np.array([np.dot(xs[i], xs[j]) for i, j in GR.pairs(n)])
    err = float(np.abs(dec[:, 0] - exp).max())
    print("inner products: max error %.3g" % err)
    assert err < 1e-6

    dist = D.gram_sq_distances(c, G, n)
    off = [(i, j) for i, j in GR.pairs(n) if i != j]
    assert dist.shape == (len(off), 2, 3, N)
    dd = D.decrypt(c, D.eval_sum(c, D.rescale(c, dist), S), len(off) * S, scale).cpu().numpy().reshape(len(off), S)
    dexp = np.array([np.sum((xs[i] - xs[j]) ** 2) for i, j in off])
    derr = float(np.abs(dd[:, 0] - dexp).max())
    print("squared distances: max error %.3g" % derr)
    assert derr < 4e-6


# ------------------------------------------------------------------- neighbours ----
def test_neighbours_give_the_same_bits_around_a_gram():
    x = chain("n13")
    c, q, N = x["c"], x["q"], x["N"]
    c.rotationKeyGen([3])
    rng = _rng("n13", 3, 11)
    a, b = (_dev(_residue_batch(rng, q, 2, 3, N)) for _ in range(2))

    def neighbours():
        return D.mult(c, a, b), D.rotate(c, a, 3), D.rescale(c, b), D.dot(c, a, b)

    before = neighbours()
    big = _dev(np.stack([_residue_batch(rng, q, 3, 3, N) for _ in range(5)]))  # a larger scratch than theirs
    D.gram(c, big)
    D.gram(c, [big[4], big[0], big[4]])
    for u, v in zip(before, neighbours()):
        assert torch.equal(u, v)
