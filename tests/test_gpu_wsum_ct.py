"""EvalLinearWSum with encrypted weights on the MI355X: device.wsum_ct -- out[k] = sum_c
w_c (x) u_{c,k} over C learners, one key switch per output ciphertext -- bit for bit against tests/wsum_ref.py
(checked for what it means by tests/test_wsum_ref.py), on raw residues, every output buffer passed in filled with
ones, the inputs checked unchanged after each call.  Chains and helpers are tests/test_gpu_gram.py's.

  learner counts      C = 1, 2, 3, 4, 5, 8, 31, 32 at 2^11 / L3, K = 3, one shared set of 32 batches: the paired
                      learner loop and its odd tail; separate tensors, views of a stack and the stack; one weight
                      ciphertext a learner (Kw = 1) and one per update ciphertext (Kw = K)
  against neighbours  every out[k] is device.dot of the stacked weights and the k-th column; C = 1 is device.mult
  chains and levels   test_gpu_gram.py's CASES at C = 3, K = 2
  level mismatch      updates stored at L towers, weights at L - 1 and at 1: the call on contiguous prefix copies
                      and the reference, the updates' unread towers filled with all-ones words
  accumulator limit   C = 32 on 60-bit and on 45- / 30-bit towers: every residue q_t - 1 (the sums are the
                      constants 32, 64, 32), and maximal w1 against uniform updates
  chunks              K = 5 in 2, 3 and 5 launch chains: the same bits, the count include/shelfi.h promises
  guards              every refusal of shelfi_dev_wsum_ct and of device.wsum_ct; a following mult is the oracle's
  meaning             wsum_ct -> rescale -> decrypt is sum_c w_c x_c, as are C mults, rescales and adds
  neighbours          mult, dot, rotate and rescale give the same bits before and after a wsum_ct"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import wsum_ref as WR
from conftest import set_switch
from f4_cases import _full_batch, _residue_batch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import test_gpu_gram as TG  # noqa: E402  (the chain table, chain(), _make(), _const_ref())
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

CHUNK = "SHELFI_EVAL_CHUNK_MIB"
chain, _dev, _u64, _rng = TG.chain, TG._dev, TG._u64, TG._rng
KW = pytest.mark.parametrize("per_k", [False, True], ids=["Kw=1", "Kw=K"])


def _ones(K, Ll, N):
    return torch.ones((K, 2, Ll, N), dtype=torch.int64, device="cuda")


def _wsum(x, us, ws, how="separate"):
    """device.wsum_ct into a buffer of ones.  how: the batches as separate allocations, as views of stacked
    tensors, or the stacked tensors themselves."""
    (K, _, _, N), Ll = us[0].shape, ws[0].shape[2]
    if how == "separate":
        tu, tw = [_dev(u) for u in us], [_dev(w) for w in ws]
        au, aw = tu, tw
    else:
        su, sw = _dev(np.stack(us)), _dev(np.stack(ws))
        tu, tw = [su[i] for i in range(len(us))], [sw[i] for i in range(len(ws))]
        au, aw = (tu, tw) if how == "views" else (su, sw)
    out = _ones(K, Ll, N)
    assert D.wsum_ct(x["c"], au, aw, out=out) is out
    for t, a in zip(tu + tw, list(us) + list(ws)):
        assert np.array_equal(_u64(t), a)  # the inputs are read only
    return _u64(out)


def _ref(x, us, ws):
    return WR.wsum_ref(us, ws, x["evk"], x["q"], x["psi"])


def _operands(x, rng, n, K, Kw, Ll, Lu=None):
    q, N = x["q"], x["N"]
    return ([_residue_batch(rng, q, K, Lu or Ll, N) for _ in range(n)],
            [_residue_batch(rng, q, Kw, Ll, N) for _ in range(n)])


# --------------------------------------------------------------- learner counts ----
LEARNERS = [1, 2, 3, 4, 5, 8, 31, 32]


@functools.lru_cache(maxsize=None)
def _learners():
    """32 uniform update batches of K = 3 at 2^11 / L3 and 32 weight batches of 3; Kw = 1 uses each one's first."""
    x = chain("n11")
    return _operands(x, _rng("n11", 3, 21), 32, 3, 3, 3)


@functools.lru_cache(maxsize=None)
def _learners_ref(n, per_k):
    us, ws = _learners()
    ws = ws[:n] if per_k else [w[:1] for w in ws[:n]]
    ref = _ref(chain("n11"), us[:n], ws)
    ref.setflags(write=False)
    return us[:n], ws, ref


@KW
@pytest.mark.parametrize("n", LEARNERS)
def test_every_learner_count(n, per_k):
    x = chain("n11")
    us, ws, ref = _learners_ref(n, per_k)
    for how in ("separate", "views", "stacked"):
        got = _wsum(x, us, ws, how)
        assert got.shape == (3, 2, 3, x["N"])
        assert np.array_equal(got, ref), how
        assert x["c"].eval_chunk_count() == 1


# ----------------------------------------------------------- against neighbours ----
@KW
def test_every_output_is_dot_of_its_column_and_one_learner_is_mult(per_k):
    x = chain("n11")
    c, n, K = x["c"], 3, 4
    us, ws = _operands(x, _rng("n11", 3, 22), n, K, K if per_k else 1, 3)
    got = _wsum(x, us, ws)
    W = [_dev(np.stack([w[k if per_k else 0] for w in ws])) for k in range(K)]
    U = [_dev(np.stack([u[k] for u in us])) for k in range(K)]
    for k in range(K):
        assert np.array_equal(_u64(D.dot(c, W[k], U[k])), got[k:k + 1]), k
    one = _wsum(x, us[:1], ws[:1])
    w = _dev(ws[0] if per_k else np.repeat(ws[0], K, axis=0))
    assert np.array_equal(_u64(D.mult(c, w, _dev(us[0]))), one)


# ------------------------------------------------------------ chains and levels ----
@KW
@pytest.mark.parametrize("cid,Ll", TG.CASES, ids=str)
def test_chains_and_levels(cid, Ll, per_k):
    x = chain(cid)
    us, ws = _operands(x, _rng(cid, Ll, 23), 3, 2, 2 if per_k else 1, Ll)
    got = _wsum(x, us, ws)
    assert got.shape == (2, 2, Ll, x["N"])
    assert np.array_equal(got, _ref(x, us, ws))


# --------------------------------------------------------------- level mismatch ----
@KW
@pytest.mark.parametrize("low", ["L-1", "1"])
@pytest.mark.parametrize("cid", ["A", "G"])
def test_updates_stored_above_the_weights_level(cid, low, per_k):
    x = chain(cid)
    L = x["L"]
    Ll = L - 1 if low == "L-1" else 1
    us, ws = _operands(x, _rng(cid, Ll, 24), 3, 2, 2 if per_k else 1, Ll, Lu=L)
    for u in us:
        u[:, :, Ll:] = np.uint64(0xFFFFFFFFFFFFFFFF)  # never read: no residue, and it would show in any sum
    got = _wsum(x, us, ws)
    assert got.shape == (2, 2, Ll, x["N"])
    assert np.array_equal(got, _wsum(x, [np.ascontiguousarray(u[:, :, :Ll]) for u in us], ws))
    assert np.array_equal(got, _ref(x, us, ws))
    assert np.array_equal(got, _wsum(x, us, ws, "stacked"))


# ------------------------------------------------------------ accumulator limit ----
@KW
@pytest.mark.parametrize("cid", ["n11", "G"])
def test_maximal_products_at_the_learner_cap(cid, per_k):
    """Every residue q_t - 1 in 32 learners: (q - 1)^2 = 1 mod q, so every output's sums are 32, 64, 32 -- the
    largest value the c1 accumulator ever holds, 64 (q - 1)^2."""
    x = chain(cid)
    L, N, K = x["L"], x["N"], 2
    full = _full_batch(x["q"], K, L, N)
    us, ws = [full] * 32, [full if per_k else full[:1]] * 32
    got = _wsum(x, us, ws, "stacked")
    ref = TG._const_ref(cid, 32)
    for k in range(K):
        assert np.array_equal(got[k:k + 1], ref), k


@KW
@pytest.mark.parametrize("cid", ["n11", "G"])
def test_maximal_w1_against_uniform_updates_at_the_learner_cap(cid, per_k):
    x = chain(cid)
    L, N, K = x["L"], x["N"], 2
    Kw = K if per_k else 1
    us, ws = _operands(x, _rng(cid, L, 25), 32, K, Kw, L)
    for w in ws:
        w[:, 1] = _full_batch(x["q"], Kw, L, N)[:, 1]
    assert np.array_equal(_wsum(x, us, ws), _ref(x, us, ws))


# ----------------------------------------------------------------------- chunks ----
@KW
def test_chains_of_outputs_do_not_change_a_bit(per_k, monkeypatch):
    """2^13 / 3 towers: a ciphertext's key-switch scratch is 29 polynomials of 2^13 words, 1.8125 MiB (and 64
    bytes), so budgets of 6, 4 and 1 MiB hold 3, 2 and 1 ciphertexts: K = 5 split evenly over the fewest chains
    runs 3 + 2, 2 + 2 + 1 and five of one (include/shelfi.h: shelfi_dev_mult's chunking)."""
    x = chain("n13")
    c, K = x["c"], 5
    us, ws = _operands(x, _rng("n13", 3, 26), 3, K, K if per_k else 1, 3)
    whole = _wsum(x, us, ws)
    assert c.eval_chunk_count() == 1
    assert np.array_equal(whole, _ref(x, us, ws))
    for mib, chains in (("6", 2), ("4", 3), ("1", 5)):
        set_switch(monkeypatch, CHUNK, mib)
        assert np.array_equal(_wsum(x, us, ws), whole), mib
        assert c.eval_chunk_count() == chains, mib
    set_switch(monkeypatch, CHUNK, None)
    assert np.array_equal(_wsum(x, us, ws, "stacked"), whole) and c.eval_chunk_count() == 1


# ----------------------------------------------------------------------- guards ----
def _mult_is_the_oracles(x, a, b):
    got = _u64(D.mult(x["c"], _dev(a), _dev(b)))
    assert np.array_equal(got, O.eval_mult(a, b, x["evk"], x["q"], x["psi"]))


def test_guards():
    x = chain("D")
    c, q, N, L = x["c"], x["q"], x["N"], x["L"]
    lib = _lib.load()
    rng = _rng("D", 4, 27)
    n, K, Lu, Ll = 3, 3, 5, 4
    us, ws = _operands(x, rng, n, K, 1, Ll, Lu=Lu)
    good = _wsum(x, us, ws)
    assert np.array_equal(good, _ref(x, us, ws))
    count = c.eval_chunk_count()
    ma = np.ascontiguousarray(us[0][:, :, :Ll])  # (an operand for the mult after each refusal)
    # one arena, in words: room for an output | the weights | the updates | room for the largest refused shape
    # behind them -- a call that should have been refused stays inside it whatever it reads or writes
    ctw, uctw, wide = 2 * Ll * N, 2 * Lu * N, 2 * (L + 1) * N
    lead, w0, u0 = 0, K * ctw, K * ctw + n * ctw
    room = u0 + n * K * uctw
    arena = torch.zeros(room + (n + 1) * K * wide, dtype=torch.int64, device="cuda")
    for i in range(n):
        arena[w0 + i * ctw:w0 + (i + 1) * ctw] = _dev(ws[i]).view(-1)
        arena[u0 + i * K * uctw:u0 + (i + 1) * K * uctw] = _dev(us[i]).view(-1)
    before = arena.clone()
    base = arena.data_ptr()
    wp = [base + 8 * (w0 + i * ctw) for i in range(n)]
    up = [base + 8 * (u0 + i * K * uctw) for i in range(n)]
    behind = [base + 8 * (room + i * K * wide) for i in range(n + 1)]  # zeros, spaced for L + 1 towers
    out = _ones(K, L + 1, N)  # (as large as the widest refused shape)
    po = out.data_ptr()
    many = torch.zeros((66, 1, 2, Ll, N), dtype=torch.int64, device="cuda")
    mp = [many[i].data_ptr() for i in range(66)]

    def raw(ups, nb, Kc, lu, wps, Kw, l, o):
        ua = None if ups is None else (C.c_void_p * len(ups))(*ups)
        wa = None if wps is None else (C.c_void_p * len(wps))(*wps)
        return lib.shelfi_dev_wsum_ct(c._ctx, ua, nb, Kc, lu, wa, Kw, l, C.c_void_p(o), None)

    def last():
        return lib.shelfi_last_error().decode()

    assert raw(up, 0, K, Lu, wp, 1, Ll, po) == _lib.SHELFI_ERR_ARG and "1..32" in last()  # C = 0 and 33, by name
    assert raw(mp[:33], 33, 1, Ll, mp[33:], 1, Ll, po) == _lib.SHELFI_ERR_ARG and "1..32" in last()
    refused = [
        lambda: raw(up, 0, K, Lu, wp, 1, Ll, po),                              # C = 0
        lambda: raw(mp[:33], 33, 1, Ll, mp[33:], 1, Ll, po),                   # C = 33
        lambda: raw(up, n, 0, Lu, wp, 1, Ll, po),                              # K = 0
        lambda: raw(up, n, 0, Lu, wp, 0, Ll, po),
        lambda: raw(up, n, K, Lu, wp, 0, Ll, po),                              # Kw not in {1, K}
        lambda: raw(up, n, K, Lu, wp, 2, Ll, po),
        lambda: raw(up, n, K, Lu, wp, K + 1, Ll, po),
        lambda: raw(up, n, K, Lu, wp, 1, 0, po),                               # towers 0
        lambda: raw(up, n, K, Lu, behind[:n], 1, Lu + 1, po),                  # towers above the updates' (<= L)
        lambda: raw(up, n, K, Ll - 1, wp, 1, Ll, po),
        lambda: raw(behind[:n], n, K, L + 1, wp, 1, Ll, po),                   # u_towers L + 1
        lambda: raw(behind[:n], n, K, L + 1, [behind[n]] * n, 1, L + 1, po),   # ... and towers with it
        lambda: raw(None, n, K, Lu, wp, 1, Ll, po),                            # NULL pointers
        lambda: raw(up, n, K, Lu, None, 1, Ll, po),
        lambda: raw([up[0], None, up[2]], n, K, Lu, wp, 1, Ll, po),
        lambda: raw(up, n, K, Lu, [wp[0], wp[1], None], 1, Ll, po),
        lambda: raw(up, n, K, Lu, wp, 1, Ll, None),
        lambda: raw(up, n, K, Lu, wp, 1, Ll, up[0]),                           # out aliasing the first update batch
        lambda: raw(up, n, K, Lu, wp, 1, Ll, up[1] + 8 * uctw),                # ... inside an inner one
        lambda: raw(up, n, K, Lu, wp, 1, Ll, up[2] + 8 * (K * uctw - (Lu - Ll) * N)),  # ... only towers never read
        lambda: raw(up, n, K, Lu, wp, 1, Ll, up[2] + 8 * (K * uctw - 1)),      # ... the last update's last word
        lambda: raw([up[1], up[2], up[2]], n, K, Lu, wp, 1, Ll, up[0] + 8 * uctw),  # out's tail in a batch given twice
        lambda: raw(up, n, K, Lu, wp, 1, Ll, wp[1]),                           # out aliasing a weight
        lambda: raw(up, n, K, Lu, wp, 1, Ll, base + 8 * (lead + N)),           # out's last N words in the first weight
        lambda: raw(up, n, K, Lu, wp, 1, Ll, wp[2] + 8 * (ctw - 1)),           # out from the last weight's last word
    ]
    for i, call in enumerate(refused):
        assert call() == _lib.SHELFI_ERR_ARG, i
        assert c.eval_chunk_count() == count, i
        assert bool((out == 1).all()) and torch.equal(arena, before) and not bool(many.any()), i
        _mult_is_the_oracles(x, ma[:1], ws[1])
        count = c.eval_chunk_count()  # (the mult's own chain count)
    # the same through device.wsum_ct
    tu = [arena[u0 + i * K * uctw:u0 + (i + 1) * K * uctw].view(K, 2, Lu, N) for i in range(n)]
    tw = [arena[w0 + i * ctw:w0 + (i + 1) * ctw].view(1, 2, Ll, N) for i in range(n)]
    wK = torch.zeros((K + 1, 2, Ll, N), dtype=torch.int64, device="cuda")
    for call in (lambda: D.wsum_ct(c, [], []),
                 lambda: D.wsum_ct(c, [many[i] for i in range(33)], [many[33 + i] for i in range(33)]),
                 lambda: D.wsum_ct(c, tu, tw[:2]),                                  # a weight batch missing
                 lambda: D.wsum_ct(c, [t[:0] for t in tu], tw),                     # K = 0
                 lambda: D.wsum_ct(c, tu, [wK[:2]] * n),                            # Kw = 2, K + 1, 0
                 lambda: D.wsum_ct(c, tu, [wK] * n),
                 lambda: D.wsum_ct(c, tu, [wK[:0]] * n),
                 lambda: D.wsum_ct(c, [t[:, :, :Ll - 1].contiguous() for t in tu], tw),   # updates below the weights
                 lambda: D.wsum_ct(c, [tu[0], tu[1][:2], tu[2]], tw),               # ragged operands
                 lambda: D.wsum_ct(c, tu, [tw[0], wK[:1, :, :2].contiguous(), tw[2]]),
                 lambda: D.wsum_ct(c, tu, tw, out=_ones(K - 1, Ll, N)),             # out of another shape or level
                 lambda: D.wsum_ct(c, tu, tw, out=_ones(K, Lu, N)),
                 lambda: D.wsum_ct(c, tu, tw, out=arena[u0:u0 + K * ctw].view(K, 2, Ll, N)),   # out in an update
                 lambda: D.wsum_ct(c, tu, tw, out=arena[w0 - (K - 1) * ctw:w0 + ctw].view(K, 2, Ll, N)),  # ... a weight
                 lambda: D.wsum_ct(c, torch.stack(tu)[:, :, :1], torch.stack(tw)),  # a stack that is not contiguous
                 lambda: D.wsum_ct(c, [t.cpu() for t in tu], tw),
                 lambda: D.wsum_ct(c, [t.view(-1) for t in tu], tw)):               # not a ciphertext tensor
        with pytest.raises(ValueError):
            call()
        assert c.eval_chunk_count() == count
    assert torch.equal(arena, before)
    _mult_is_the_oracles(x, ma, np.repeat(ws[1], K, axis=0))
    tail = arena[room:room + K * ctw].view(K, 2, Ll, N)
    assert np.array_equal(_u64(D.wsum_ct(c, tu, tw, out=tail)), good)


def test_no_evaluation_key_is_a_state_error():
    x = TG._make(1 << 11, 3, 52, 60, 1651)
    c, N = x["c"], x["N"]
    us, ws = _operands(x, np.random.default_rng(28), 2, 2, 1, 3)
    out = _ones(2, 3, N)
    with pytest.raises(RuntimeError, match="evaluation key") as e:
        D.wsum_ct(c, [_dev(u) for u in us], [_dev(w) for w in ws], out=out)
    assert e.value.code == _lib.SHELFI_ERR_STATE
    assert torch.equal(out, _ones(2, 3, N)) and c.eval_chunk_count() == 0
    c.evalMultKeyGen()
    x["evk"] = c.get_eval_key()
    _mult_is_the_oracles(x, us[0], us[1])
    assert np.array_equal(_wsum(x, us, ws), _ref(x, us, ws))


def test_chain_too_long_is_refused_by_name():
    """tests/f4_cases.py's 13-tower chain: 5 special primes, 18 towers; no key can exist, and the call says why
    rather than asking for one."""
    x = TG._make(1 << 12, 13, 52, 60, 1613)
    c, q, N = x["c"], x["q"], x["N"]
    assert len(O.special_primes(N, q)[2]) == 5
    a = _dev(_residue_batch(np.random.default_rng(29), q, 2, 13, N))
    low = a[:, :, :2].contiguous()
    for call in (lambda: D.wsum_ct(c, [a, a], [a[:1], a[1:]]), lambda: D.wsum_ct(c, [a, a], [low, low])):
        with pytest.raises(ValueError, match="<= 16"):
            call()
    assert c.eval_chunk_count() == 0 and not c.eval_key_info()["has_key"]


# ---------------------------------------------------------------------- meaning ----
def test_wsum_rescale_decrypts_to_the_weighted_sum():
    """2^12 / L3, C = 3 learners of K = 2 ciphertexts of 2048 slots, weights in (0, 1): a constant a learner
    (Kw = 1), then (Kw = K) a constant for the first ciphertext and a per-slot vector for the second.  After
    ModReduce every slot holds sum_c w_c x_c; C mults, ModReduces and adds reach the same numbers with C key-switch
    errors an output where wsum_ct has one.  The bound is test_gpu_dot.py's on this ring and chain, held there
    for a sum over 8192 products."""
    x = TG._make(1 << 12, 3, 52, 60, 1661)
    c, q, N, inf = x["c"], x["q"], x["N"], x["inf"]
    c.evalMultKeyGen()
    S, K, n = inf["batch"], 2, 3
    rng = np.random.default_rng(30)
    xs = rng.uniform(-1, 1, (n, K, S))
    wc = rng.uniform(0, 1, (n, 1, 1)) * np.ones((n, 1, S))
    wv = np.concatenate([wc, rng.uniform(0, 1, (n, 1, S))], axis=1)  # [n][K][S]: a constant, then per slot

    def enc(v):
        return D.encrypt(c, torch.tensor(v.reshape(-1), dtype=torch.float64, device="cuda"))

    us = [enc(v) for v in xs]
    assert us[0].shape == (K, 2, 3, N)
    scale = inf["delta"] * inf["delta"] / float(q[2])
    for name, wvals in (("Kw = 1", wc), ("Kw = K", wv)):
        ws = [enc(v) for v in wvals]
        Kw = wvals.shape[1]
        assert ws[0].shape == (Kw, 2, 3, N)
        exp = (wvals * xs).sum(axis=0).reshape(-1)
        out = D.wsum_ct(c, us, ws)
        assert out.shape == (K, 2, 3, N)
        dec = D.decrypt(c, D.rescale(c, out), K * S, scale).cpu().numpy()
        err = float(np.abs(dec - exp).max())
        acc = None
        for u, w in zip(us, ws):
            prod = D.rescale(c, D.mult(c, w if Kw == K else w.repeat(K, 1, 1, 1), u))
            acc = prod if acc is None else D.add(c, acc, prod, out=acc)
        err_par = float(np.abs(D.decrypt(c, acc, K * S, scale).cpu().numpy() - exp).max())
        print("%s: wsum_ct error %.3g, per-learner path error %.3g" % (name, err, err_par))
        assert err < 1e-6 and err_par < 1e-6


# ------------------------------------------------------------------- neighbours ----
def test_neighbours_give_the_same_bits_around_a_wsum_ct():
    x = chain("n13")
    c, q, N = x["c"], x["q"], x["N"]
    c.rotationKeyGen([3])
    rng = _rng("n13", 3, 31)
    a, b = (_dev(_residue_batch(rng, q, 2, 3, N)) for _ in range(2))

    def neighbours():
        return D.mult(c, a, b), D.dot(c, a, b), D.rotate(c, a, 3), D.rescale(c, b)

    before = neighbours()
    big = _dev(np.stack([_residue_batch(rng, q, 4, 3, N) for _ in range(5)]))  # a larger scratch than theirs
    D.wsum_ct(c, big, big[:, :1].contiguous())
    D.wsum_ct(c, [big[4], big[0]], [big[1], big[1]])
    for u, v in zip(before, neighbours()):
        assert torch.equal(u, v)
