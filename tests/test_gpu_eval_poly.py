"""EvalPoly on the MI355X: device.poly_combine / shelfi_dev_poly_combine -- every giant-step
product of Paterson-Stockmeyer summed as one tensor, one key switch per output ciphertext -- and device.eval_poly,
bit for bit against tests/poly_ref.py (checked for what it means by tests/test_poly_ref.py and, for the plan, by
tests/test_poly_plan.py), on raw residues, every output buffer passed in filled with ones, the inputs checked
unchanged after each call.  Chains and helpers are tests/test_gpu_gram.py's.

  every shape         degrees 1..31 at 2^11 / L3, K = 3: every (babies, giants) pair a degree produces, and the pairs
                      only the C entry reaches (1 or 2 babies with giants); uniform operands, every W arbitrary in
                      [0, q); no giants on a context WITHOUT an evaluation key
  chains and levels   test_gpu_gram.py's CASES and 2^13 / L3 at degrees 7 and 13, K = 2 (2^15 / L4 at K = 1)
  level mismatch      babies stored at L, L - 1, L - 2 and giants at L - 2 and L, the unread towers all-ones words:
                      the call on contiguous prefix copies and the reference
  accumulator limit   7 giants, 3 babies on 60-bit and 45- / 30-bit towers: every residue and every W q_t - 1, and
                      constants chosen so that every q_{g,.} reduces to q_t - 1 and every giant-step product is
                      (q - 1)^2; the closed-form constants through the relinearization reference
  neighbours          W_{0,1} = 1 alone returns P_1's prefix; W_{1,1} = 1 alone is wsum_ct([P_1], [P_4]); without
                      giants the result is mult_plain by constant plaintexts plus add; mult, dot, rotate and rescale
                      give the same bits before and after an eval_poly
  chunks              K = 5 in 2, 3 and 5 launch chains: the same bits, the count include/shelfi.h promises
  guards              every refusal of shelfi_dev_poly_combine and of device.eval_poly / poly_powers / poly_combine;
                      a following mult is the oracle's
  whole call          device.eval_poly on encrypted data at chain "A", degrees 3 and 7: poly_ref's pipeline bit for
                      bit, numpy.polyval within test_poly_ref.py's recorded tolerance
  clipping            dot(u, u) -> rescale -> eval_sum -> eval_poly -> wsum_ct -> rescale -> decrypt"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import poly_ref as PR
import test_poly_ref as TPR
from conftest import set_switch
from f4_cases import _full_batch, _residue_batch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import test_gpu_gram as TG  # noqa: E402  (the chain table, chain(), _make())
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

CHUNK = "SHELFI_EVAL_CHUNK_MIB"
chain, _dev, _u64, _rng = TG.chain, TG._dev, TG._u64, TG._rng
FILL = np.uint64(0xFFFFFFFFFFFFFFFF)


def _ones(K, Ll, N):
    return torch.ones((K, 2, Ll, N), dtype=torch.int64, device="cuda")


def _table(rng, q, ng, towers):
    """[ng + 1][4][towers] uniform residues: every W arbitrary in [0, q_t)."""
    return rng.integers(0, np.array([int(v) for v in q[:towers]], np.uint64), size=(ng + 1, 4, towers), dtype=np.uint64)


def _operands(x, rng, nb, ng, K, towers, stored=None):
    q, N = x["q"], x["N"]
    stored = stored or [towers] * (nb + ng)
    ops = [_residue_batch(rng, q, K, s, N) for s in stored]
    return ops[:nb], ops[nb:], _table(rng, q, ng, towers)


def _combine(x, babies, giants, table, towers, c=None):
    """device.poly_combine into a buffer of ones; the operands are read only."""
    K, N = babies[0].shape[0], x["N"]
    tb, tg = [_dev(v) for v in babies], [_dev(v) for v in giants]
    out = _ones(K, towers, N)
    assert D.poly_combine(c or x["c"], tb, tg, table, towers, out=out) is out
    for t, a in zip(tb + tg, list(babies) + list(giants)):
        assert np.array_equal(_u64(t), a)
    return _u64(out)


def _ref(x, babies, giants, table, towers):
    return PR.combine_ref(babies, giants, table, towers, x["evk"], x["q"], x["psi"])


# ------------------------------------------------------------------ every shape ----
@functools.lru_cache(maxsize=None)
def _pool():
    """10 uniform batches of K = 3 at 2^11 / L3: the first 3 serve as babies, the rest as giants."""
    x = chain("n11")
    rng = _rng("n11", 3, 41)
    return [_residue_batch(rng, x["q"], 3, 3, x["N"]) for _ in range(10)]


@functools.lru_cache(maxsize=None)
def _nokey():
    return TG._make(1 << 11, 3, 52, 60, 1671)  # no evaluation key, ever


def _shape(nb, ng, salt):
    x = chain("n11")
    ops = _pool()
    babies, giants = ops[:nb], ops[3:3 + ng]
    table = _table(_rng("n11", 3, 1000 + salt), x["q"], ng, 3)
    got = _combine(x, babies, giants, table, 3)
    assert got.shape == (3, 2, 3, x["N"])
    assert np.array_equal(got, _ref(x, babies, giants, table, 3)), (nb, ng)
    assert x["c"].eval_chunk_count() == 1
    if not ng:  # no tensor, no key switch: a context that has no evaluation key gives the same bits
        y = _nokey()
        assert np.array_equal(y["q"], x["q"]) and not y["c"].eval_key_info()["has_key"]
        assert np.array_equal(_combine(x, babies, giants, table, 3, c=y["c"]), got)


@pytest.mark.parametrize("d", range(1, 32))
def test_every_degree(d):
    _shape(min(d, 3), (d + 4) // 4 - 1, d)


@pytest.mark.parametrize("nb,ng", [(nb, ng) for nb in (1, 2) for ng in range(1, 8)])
def test_pairs_no_degree_produces(nb, ng):
    _shape(nb, ng, 100 + 10 * nb + ng)


# ------------------------------------------------------------ chains and levels ----
@pytest.mark.parametrize("d", [7, 13])
@pytest.mark.parametrize("cid,Ll", TG.CASES + [("n13", 3)], ids=str)
def test_chains_and_levels(cid, Ll, d):
    x = chain(cid)
    K = 1 if cid == "n15" else 2
    nb, ng = 3, (d + 4) // 4 - 1
    babies, giants, table = _operands(x, _rng(cid, Ll, 42 + d), nb, ng, K, Ll)
    got = _combine(x, babies, giants, table, Ll)
    assert got.shape == (K, 2, Ll, x["N"])
    assert np.array_equal(got, _ref(x, babies, giants, table, Ll))


# --------------------------------------------------------------- level mismatch ----
@pytest.mark.parametrize("cid", ["A", "G"])
def test_operands_stored_above_the_combine_level(cid):
    x = chain(cid)
    L = x["L"]
    t = L - 2
    stored = [L, L - 1, L - 2, L - 2, L, L - 2]  # P_1, P_2, P_3 | P_4, P_8, P_12
    babies, giants, table = _operands(x, _rng(cid, t, 43), 3, 3, 2, t, stored)
    for v in babies + giants:
        v[:, :, t:] = FILL  # never read: no residue, and it would show in any sum
    got = _combine(x, babies, giants, table, t)
    assert got.shape == (2, 2, t, x["N"])
    cut = lambda vs: [np.ascontiguousarray(v[:, :, :t]) for v in vs]  # noqa: E731
    assert np.array_equal(got, _combine(x, cut(babies), cut(giants), table, t))
    assert np.array_equal(got, _ref(x, babies, giants, table, t))
    # the same without giants, where the other kernel runs
    got0 = _combine(x, babies, [], table[:1], t)
    assert np.array_equal(got0, _combine(x, cut(babies), [], table[:1], t))
    assert np.array_equal(got0, _ref(x, babies, [], table[:1], t))


# ------------------------------------------------------------ accumulator limit ----
def _constant_tensor_ref(x, d0, d1, d2):
    """[1][2][L][N]: (d0, d1) + KeySwitch(d2) for tensors that hold the constants d0, d1, d2 (mod q_t) at every
    evaluation point, through the relinearization reference."""
    q, L, N = x["q"], x["L"], x["N"]
    Xc, Y, d01 = (np.zeros((1, 2, L, N), np.uint64) for _ in range(3))
    for t in range(L):
        d01[0, 0, t], d01[0, 1, t], Xc[0, 1, t] = d0 % int(q[t]), d1 % int(q[t]), d2 % int(q[t])
    Y[:, 1] = 1
    return (O.eval_mult(Xc, Y, x["evk"], q, x["psi"]) + d01) % np.asarray(q[:L], np.uint64)[None, None, :, None]


@pytest.mark.parametrize("cid", ["n11", "g11"])
def test_every_residue_and_constant_maximal(cid):
    """The issue's case: every residue and every W is q_t - 1 = -1, so q_{g,0} = -1 + 3 = 2 and q_{g,1} = 3, and with
    7 giants d0 = 2 - 14, d1 = 3 - 7 (3 + 2), d2 = -21.  Every baby-step product (the q_{g,.} sums, d0's and d1's
    first three) is (q - 1)^2; the giant-step products are (q - 1) times 2 or 3 -- the next test makes those
    maximal too."""
    x = chain(cid)
    q, L, N, K = x["q"], x["L"], x["N"], 2
    full = _full_batch(q, K, L, N)
    table = np.stack([[np.array([int(v) - 1 for v in q[:L]], np.uint64)] * 4] * 8)
    got = _combine(x, [full] * 3, [full] * 7, table, L)
    ref = _constant_tensor_ref(x, -12, -32, -21)
    for k in range(K):
        assert np.array_equal(got[k:k + 1], ref), k
    assert np.array_equal(got, _ref(x, [full] * 3, [full] * 7, table, L))


@pytest.mark.parametrize("cid", ["n11", "g11"])
def test_maximal_giant_step_products(cid):
    """The accumulators at their longest runs of maximal products.  W_{g,0} = q - 4 and W_{g,j} = q - 1 against
    babies of q - 1 give q_{g,0} = -4 + 3 = -1; P_3's second component is 3 instead, so q_{g,1} = 1 + 1 - 3 = -1.
    Both reduce to q - 1, and with every giant residue q - 1 all 7 products into d0, all 14 into d1 and all 7 into
    d2 are (q - 1)^2 -- d1 holding 2 (q - 1)^2 + 3 (q - 1) + 14 (q - 1)^2, one short of its 17.  d0 = -1 + 7,
    d1 = -1 + 14, d2 = 7."""
    x = chain(cid)
    q, L, N, K = x["q"], x["L"], x["N"], 2
    full = _full_batch(q, K, L, N)
    p3 = full.copy()
    p3[:, 1] = 3
    table = np.stack([[np.array([int(v) - w for v in q[:L]], np.uint64) for w in (4, 1, 1, 1)]] * 8)
    got = _combine(x, [full, full, p3], [full] * 7, table, L)
    ref = _constant_tensor_ref(x, 6, 13, 7)
    for k in range(K):
        assert np.array_equal(got[k:k + 1], ref), k
    assert np.array_equal(got, _ref(x, [full, full, p3], [full] * 7, table, L))


# ------------------------------------------------------------------- neighbours ----
def test_one_unit_constant_returns_the_operand_or_the_product():
    x = chain("A")
    c, q, N, t = x["c"], x["q"], x["N"], 4
    rng = _rng("A", t, 44)
    p1, p4 = _residue_batch(rng, q, 2, 6, N), _residue_batch(rng, q, 2, 4, N)
    tab = np.zeros((1, 4, t), np.uint64)
    tab[0, 1] = 1
    assert np.array_equal(_combine(x, [p1], [], tab, t), p1[:, :, :t])           # (a) W_{0,1} = 1: P_1's prefix
    tab = np.zeros((2, 4, t), np.uint64)
    tab[1, 1] = 1
    got = _combine(x, [p1], [p4], tab, t)                                         # (b) W_{1,1} = 1: P_4 (x) P_1
    assert np.array_equal(got, _u64(D.wsum_ct(c, [_dev(p1)], [_dev(p4)])))
    assert np.array_equal(got, _ref(x, [p1], [p4], tab, t))


def test_without_giants_it_is_mult_plain_and_add():
    x = chain("A")
    c, q, N, t, K = x["c"], x["q"], x["N"], 5, 2
    babies, _, tab = _operands(x, _rng("A", t, 45), 3, 0, K, t)
    got = _combine(x, babies, [], tab, t)
    const = lambda j: _dev(np.repeat(tab[0, j][:, None], N, axis=1)[None])  # noqa: E731  [1][t][N]: W at every point
    acc = None
    for j, b in enumerate(babies):
        term = D.mult_plain(c, _dev(b), const(1 + j))
        acc = term if acc is None else D.add(c, acc, term, out=acc)
    acc = D.add_plain(c, acc, const(0), out=acc)
    assert np.array_equal(got, _u64(acc))


def test_neighbours_give_the_same_bits_around_an_eval_poly():
    x = chain("n13")
    c, q, N = x["c"], x["q"], x["N"]
    c.rotationKeyGen([3])
    rng = _rng("n13", 3, 46)
    a, b = (_dev(_residue_batch(rng, q, 2, 3, N)) for _ in range(2))

    def neighbours():
        return D.mult(c, a, b), D.dot(c, a, b), D.rotate(c, a, 3), D.rescale(c, b)

    before = neighbours()
    big = _dev(_residue_batch(rng, q, 6, 3, N))  # a larger scratch than theirs
    D.eval_poly(c, big, [0.5, 1.0, -0.25], float(q[2]))
    D.poly_combine(c, [big, big], [big], _table(rng, q, 1, 3), 3)
    for u, v in zip(before, neighbours()):
        assert torch.equal(u, v)


# ----------------------------------------------------------------------- chunks ----
def test_chains_of_outputs_do_not_change_a_bit(monkeypatch):
    """2^13 / 3 towers: a ciphertext's key-switch scratch is 1.8125 MiB (and 64 bytes), so budgets of 6, 4 and 1 MiB
    hold 3, 2 and 1 ciphertexts: K = 5 runs 3 + 2, 2 + 2 + 1 and five of one (tests/test_gpu_wsum_ct.py's split)."""
    x = chain("n13")
    c, K = x["c"], 5
    babies, giants, table = _operands(x, _rng("n13", 3, 47), 3, 2, K, 3)
    whole = _combine(x, babies, giants, table, 3)
    assert c.eval_chunk_count() == 1
    assert np.array_equal(whole, _ref(x, babies, giants, table, 3))
    for mib, chains in (("6", 2), ("4", 3), ("1", 5)):
        set_switch(monkeypatch, CHUNK, mib)
        assert np.array_equal(_combine(x, babies, giants, table, 3), whole), mib
        assert c.eval_chunk_count() == chains, mib
    set_switch(monkeypatch, CHUNK, None)
    assert np.array_equal(_combine(x, babies, giants, table, 3), whole) and c.eval_chunk_count() == 1


# ----------------------------------------------------------------------- guards ----
def _mult_is_the_oracles(x, a, b):
    got = _u64(D.mult(x["c"], _dev(a), _dev(b)))
    assert np.array_equal(got, O.eval_mult(a, b, x["evk"], x["q"], x["psi"]))


def test_guards():
    x = chain("D")
    c, q, N, L = x["c"], x["q"], x["N"], x["L"]
    lib = _lib.load()
    rng = _rng("D", 4, 48)
    K, t = 2, 4
    stored = [6, 5, 4, 4, 5]  # P_1, P_2, P_3 | P_4, P_8
    babies, giants, table = _operands(x, rng, 3, 2, K, t, stored)
    good = _combine(x, babies, giants, table, t)
    assert np.array_equal(good, _ref(x, babies, giants, table, t))
    count = c.eval_chunk_count()
    # one arena, in words: room for an output | the five operands | zeros behind them wide enough for L + 1 towers
    ctw, wide = 2 * t * N, 2 * (L + 1) * N
    offs, o = [], K * ctw
    for s in stored:
        offs.append(o)
        o += K * 2 * s * N
    room = o
    arena = torch.zeros(room + 5 * K * wide, dtype=torch.int64, device="cuda")
    for off, v in zip(offs, babies + giants):
        arena[off:off + v.size] = _dev(v).view(-1)
    before = arena.clone()
    base = arena.data_ptr()
    ptr = [base + 8 * off for off in offs]
    bp, gp, bt, gt = ptr[:3], ptr[3:], stored[:3], stored[3:]
    behind = [base + 8 * (room + i * K * wide) for i in range(5)]
    out = _ones(K, L + 1, N)
    po = out.data_ptr()
    tabp = table.ctypes.data_as(_lib.u64p)
    big = table.copy()
    big[1, 2, 3] = q[3]  # a constant at its modulus
    bigp = big.ctypes.data_as(_lib.u64p)

    def raw(bps, bts, nb, gps, gts, ng, tab, Kc, tw, o):
        ba = None if bps is None else (C.c_void_p * 3)(*bps)
        ga = None if gps is None else (C.c_void_p * 7)(*gps)
        bta = None if bts is None else (C.c_uint32 * 3)(*bts)
        gta = None if gts is None else (C.c_uint32 * 7)(*gts)
        return lib.shelfi_dev_poly_combine(c._ctx, ba, bta, nb, ga, gta, ng, tab, Kc, tw, C.c_void_p(o), None)

    def last():
        return lib.shelfi_last_error().decode()

    assert raw(bp, bt, 0, gp, gt, 2, tabp, K, t, po) == _lib.SHELFI_ERR_ARG and "1..3" in last()
    assert raw(bp, bt, 3, gp, gt, 8, tabp, K, t, po) == _lib.SHELFI_ERR_ARG and "0..7" in last()
    sz = [K * 2 * s * N for s in stored]
    refused = [
        lambda: raw(bp, bt, 0, gp, gt, 2, tabp, K, t, po),                         # nb = 0, 4
        lambda: raw(bp, bt, 4, gp, gt, 2, tabp, K, t, po),
        lambda: raw(bp, bt, 3, gp, gt, 8, tabp, K, t, po),                         # ng = 8
        lambda: raw(bp, bt, 3, gp, gt, 2, tabp, 0, t, po),                         # K = 0
        lambda: raw(bp, bt, 1, gp, gt, 0, tabp, 0, t, po),
        lambda: raw(bp, bt, 3, gp, gt, 2, tabp, K, 0, po),                         # towers 0, L + 1
        lambda: raw(behind[:3], [L + 1] * 3, 3, behind[3:], [L + 1] * 2, 2, tabp, K, L + 1, po),
        lambda: raw(bp, bt, 3, gp, gt, 2, tabp, K, 5, po),                         # operands stored below `towers`
        lambda: raw(bp, [6, 5, 3], 3, gp, gt, 2, tabp, K, t, po),
        lambda: raw(bp, bt, 3, gp, [3, 5], 2, tabp, K, t, po),
        lambda: raw(bp, bt, 3, gp, gt, 0, tabp, K, 5, po),                         # ... without giants too
        lambda: raw(behind[:3], [L + 1, 5, 4], 3, gp, gt, 2, tabp, K, t, po),      # an operand stored above L
        lambda: raw(bp, bt, 3, behind[3:], [4, L + 1], 2, tabp, K, t, po),
        lambda: raw(None, bt, 3, gp, gt, 2, tabp, K, t, po),                       # NULL pointers
        lambda: raw(bp, None, 3, gp, gt, 2, tabp, K, t, po),
        lambda: raw(bp, bt, 3, None, gt, 2, tabp, K, t, po),
        lambda: raw(bp, bt, 3, gp, None, 2, tabp, K, t, po),
        lambda: raw([bp[0], None, bp[2]], bt, 3, gp, gt, 2, tabp, K, t, po),
        lambda: raw(bp, bt, 3, [gp[0], None], gt, 2, tabp, K, t, po),
        lambda: raw(bp, bt, 3, gp, gt, 2, None, K, t, po),
        lambda: raw(bp, bt, 3, gp, gt, 2, tabp, K, t, None),
        lambda: raw(bp, bt, 3, gp, gt, 2, tabp, K, t, bp[0]),                      # out aliasing P_1
        lambda: raw(bp, bt, 3, gp, gt, 2, tabp, K, t, bp[0] + 8 * (sz[0] - 2 * N)),   # ... only towers never read
        lambda: raw(bp, bt, 3, gp, gt, 2, tabp, K, t, bp[1] + 8 * (sz[1] - 1)),    # ... P_2's last word
        lambda: raw(bp, bt, 3, gp, gt, 2, tabp, K, t, gp[0]),                      # ... a giant
        lambda: raw(bp, bt, 3, gp, gt, 2, tabp, K, t, gp[1] + 8 * (sz[4] - 1)),
        lambda: raw(bp, bt, 3, gp, gt, 2, tabp, K, t, base + 8 * N),               # out's tail in P_1
        lambda: raw(bp, bt, 3, gp, gt, 0, tabp, K, t, bp[2]),                      # ... without giants too
        lambda: raw(bp, bt, 3, gp, gt, 2, bigp, K, t, po),                         # a constant >= its modulus
    ]
    for i, call in enumerate(refused):
        assert call() == _lib.SHELFI_ERR_ARG, i
        assert c.eval_chunk_count() == count, i
        assert bool((out == 1).all()) and torch.equal(arena, before), i
        _mult_is_the_oracles(x, babies[2][:1], giants[0][:1])
        count = c.eval_chunk_count()
    # the same through the device module
    tb = [arena[off:off + n].view(K, 2, s, N) for off, n, s in zip(offs[:3], sz[:3], stored[:3])]
    tg = [arena[off:off + n].view(K, 2, s, N) for off, n, s in zip(offs[3:], sz[3:], stored[3:])]
    s1 = float(q[L - 1])
    ct = tb[0]
    for call in (lambda: D.poly_combine(c, [], tg, table, t),
                 lambda: D.poly_combine(c, tb + tb[:1], tg, table, t),
                 lambda: D.poly_combine(c, tb, tg * 4, table, t),
                 lambda: D.poly_combine(c, tb, tg, table[:2], t),                   # a table of another shape
                 lambda: D.poly_combine(c, tb, tg, table, 5),
                 lambda: D.poly_combine(c, tb, tg, table, 0),
                 lambda: D.poly_combine(c, [v[:0] for v in tb], [v[:0] for v in tg], table, t),   # K = 0
                 lambda: D.poly_combine(c, [tb[0][:1].contiguous()] + tb[1:], tg, table, t),      # ragged
                 lambda: D.poly_combine(c, tb, tg, table, t, out=_ones(K, 5, N)),
                 lambda: D.poly_combine(c, tb, tg, table, t, out=_ones(K + 1, t, N)),
                 lambda: D.poly_combine(c, tb, tg, table, t, out=arena[offs[3]:offs[3] + K * ctw].view(K, 2, t, N)),
                 lambda: D.poly_combine(c, tb, tg, big, t),
                 lambda: D.poly_combine(c, [v.cpu() for v in tb], tg, table, t),
                 lambda: D.eval_poly(c, ct, [1.0], s1),                             # degree 0 and 32
                 lambda: D.eval_poly(c, ct, [1.0] * 33, s1),
                 lambda: D.eval_poly(c, ct, [1.0, float("nan")], s1),
                 lambda: D.eval_poly(c, ct, [1.0] * 17, s1),                        # 6 towers hold no degree 16
                 lambda: D.eval_poly(c, tb[2], [1.0] * 8, s1),                      # nor 4 towers degree 7
                 lambda: D.eval_poly(c, ct, [1e300, 1.0], s1),                      # |W| >= Q / 2
                 lambda: D.eval_poly(c, ct, [1.0, 1.0], 0.0),
                 lambda: D.eval_poly(c, ct[:0], [1.0, 1.0], s1),
                 lambda: D.eval_poly(c, ct.view(-1), [1.0, 1.0], s1),
                 lambda: D.poly_powers(c, ct, s1, 0),
                 lambda: D.poly_powers(c, ct, s1, 32),
                 lambda: D.poly_powers(c, ct[:0], s1, 3),
                 lambda: D.poly_powers(c, tb[2], s1, 7)):
        with pytest.raises(ValueError):
            call()
        assert c.eval_chunk_count() == count
    assert torch.equal(arena, before)
    _mult_is_the_oracles(x, babies[2], giants[0])
    tail = arena[room:room + K * ctw].view(K, 2, t, N)
    assert np.array_equal(_u64(D.poly_combine(c, tb, tg, table, t, out=tail)), good)


def test_no_evaluation_key_is_a_state_error_with_giants_only():
    x = TG._make(1 << 11, 3, 52, 60, 1672)
    c, N = x["c"], x["N"]
    babies, giants, table = _operands(x, np.random.default_rng(49), 2, 1, 2, 3)
    out = _ones(2, 3, N)
    with pytest.raises(RuntimeError, match="evaluation key") as e:
        D.poly_combine(c, [_dev(v) for v in babies], [_dev(v) for v in giants], table, 3, out=out)
    assert e.value.code == _lib.SHELFI_ERR_STATE
    assert torch.equal(out, _ones(2, 3, N)) and c.eval_chunk_count() == 0
    with pytest.raises(RuntimeError, match="evaluation key"):
        D.eval_poly(c, _dev(babies[0]), [1.0, 1.0, 1.0], float(x["q"][2]))
    lin, s = D.eval_poly(c, _dev(babies[0]), [0.5, 1.0], float(x["q"][2]))   # degree 1 needs none
    assert lin.shape == (2, 2, 2, N) and s == 2.0 ** 104 / float(x["q"][2])
    c.evalMultKeyGen()
    x["evk"] = c.get_eval_key()
    assert np.array_equal(_combine(x, babies, giants, table, 3), _ref(x, babies, giants, table, 3))


def test_chain_too_long_is_refused_by_name():
    """tests/f4_cases.py's 13-tower chain: 5 special primes, 18 towers; no key can exist, and the call says why;
    without giants nothing is switched and the call runs."""
    x = TG._make(1 << 12, 13, 52, 60, 1613)
    c, q, N = x["c"], x["q"], x["N"]
    a = _residue_batch(np.random.default_rng(50), q, 1, 13, N)
    tab = _table(np.random.default_rng(51), q, 1, 2)
    with pytest.raises(ValueError, match="<= 16"):
        D.poly_combine(c, [_dev(a)], [_dev(a)], tab, 2)
    assert c.eval_chunk_count() == 0
    assert np.array_equal(_combine(x, [a], [], tab[:1], 2), PR.combine_ref([a], [], tab[:1], 2, None, q, x["psi"]))


# ------------------------------------------------------------------- whole call ----
@pytest.mark.parametrize("d", [3, 7])
def test_eval_poly_on_encrypted_data(d):
    x = chain("A")
    c, q, psi, N, inf = x["c"], x["q"], x["psi"], x["N"], x["inf"]
    S, K = inf["batch"], 2
    vals = np.random.default_rng([d, 52]).uniform(-1, 1, K * S)
    ct = D.encrypt(c, torch.tensor(vals, dtype=torch.float64, device="cuda"))
    assert ct.shape == (K, 2, 7, N)
    keep = ct.clone()
    coeffs = TPR.COEFFS[d]
    out, scale = D.eval_poly(c, ct, coeffs, inf["delta"])
    assert torch.equal(ct, keep)
    ref, rscale = PR.eval_poly_ref(_u64(ct), coeffs, inf["delta"], inf["scale_bits"], x["evk"], q, psi)
    assert out.shape == ref.shape == (K, 2, 7 - (3 if d == 3 else 4), N) and scale == rscale
    assert np.array_equal(_u64(out), ref)
    have = D.poly_powers(c, ct, inf["delta"], d)
    pl = PR.plan(q, inf["scale_bits"], coeffs, 7, inf["delta"])
    rp = PR.powers_ref(_u64(ct), pl, x["evk"], q, psi)
    assert sorted(have) == sorted(rp)
    for n, (t, s) in have.items():
        assert np.array_equal(_u64(t), rp[n]), n
        assert s == [p["scale"] for p in pl["powers"] if p["n"] == n][0]
    dec = D.decrypt(c, out, K * S, scale).cpu().numpy()
    err = float(np.abs(dec - np.polyval(coeffs[::-1], vals)).max())
    print("degree %d: max error %.3g (tolerance %.3g)" % (d, err, TPR.TOL[d]))
    assert err < TPR.TOL[d]


# --------------------------------------------------------------------- clipping ----
def test_private_norm_clipping_walk_through():
    """INTEGRATION.md's walk-through on chain "A": 2 learners x 2 ciphertexts.  The server never sees a norm:
    n_i = eval_sum(rescale(dot(u_i, u_i))) holds ||u_i||^2 in every slot, f_i = eval_poly(n_i) the clipping factor
    (a cubic here), and wsum_ct multiplies the updates at 7 towers by the factors at 3.
    Tolerance: 4 x the error tests/test_poly_ref.py measured for the same walk-through restated over the oracle on
    the same updates (fresh encryption noise differs by seed); both figures are in DESIGN.md 2.20."""
    x = chain("A")
    c, q, N, inf = x["c"], x["q"], x["N"], x["inf"]
    c.evalSumKeyGen()
    S, K, n = inf["batch"], 2, 2
    delta = inf["delta"]
    us, exp = TPR.clipping_inputs()                                      # ||u||^2 about 0.36 and 0.81
    assert us.shape == (n, K * S)
    coeffs = TPR.COEFFS[3]
    cts = [D.encrypt(c, torch.tensor(u, dtype=torch.float64, device="cuda")) for u in us]
    factors = []
    for ct in cts:
        nrm = D.eval_sum(c, D.rescale(c, D.dot(c, ct, ct)), S)          # [1][2][6][N] at delta^2 / q_6
        f, fs = D.eval_poly(c, nrm, coeffs, delta * delta / float(q[6]))
        assert f.shape == (1, 2, 3, N)
        factors.append(f)
    out = D.rescale(c, D.wsum_ct(c, cts, factors))                       # updates at 7 towers, factors at 3
    assert out.shape == (K, 2, 2, N)
    dec = D.decrypt(c, out, K * S, delta * fs / float(q[2])).cpu().numpy()
    err = float(np.abs(dec - exp).max())
    print("clipping: max error %.3g (tolerance %.3g)" % (err, TPR.CLIP_TOL))
    assert err < TPR.CLIP_TOL
