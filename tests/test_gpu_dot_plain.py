"""EvalInnerProduct(ct, pt) on the MI355X: device.project -- the projections of C encrypted
batches on R plaintext batches -- with device.dot_plain and device.pack_slots, bit for bit against
tests/dotp_ref.py (checked for what it means by tests/test_dotp_ref.py), on raw residues, every output buffer
passed in filled with ones.

  tile geometry       C = 1..5 x R = 1..5 at 2^11 / L3: every full and ragged tile of the 2 x 2 tiling and the
                      4 / 2 / 1 tiling of R = 1, one reference shared; 16 x 1 and 1 x 16; the batches as separate
                      tensors, as views of a stack and as the stack; one tensor at two indices
  dot_plain           project's entry 0, and mult_plain at K = 1
  rings and chains    the rings, tower counts and levels of tests/test_gpu_dot.py, C = R = K = 2
  fold edges          every residue q_t - 1 (every product maximal) in ONE slice, K straddling 128, 256 and 512
                      ciphertexts on 60- / 52- / 53-bit and on 45- / 31- / 30-bit towers: (q - 1)^2 = 1 mod q, so
                      every sum is the constant K
  slices              no output bit depends on SHELFI_DOTP_SLICE_CTS or SHELFI_EVAL_CHUNK_MIB; the counter says
                      what include/shelfi.h says
  keys                none is needed: a context without an evaluation key, and one that never had keys
  guards              every refusal of shelfi_dev_project; the calls after it are still right
  meaning             project -> rescale -> eval_sum -> decrypt is <x_c, g_r>; gram -> rescale -> eval_sum ->
                      pack_slots -> ONE decrypt opens the whole Gram matrix
  neighbours          mult_plain, dot, gram and mult give the same bits before and after a project"""
import ctypes as C
import functools

import numpy as np
import pytest

import dotp_ref as PJ
import oracle as O
import plain_ref as PR
from conftest import set_switch
from f4_cases import _full_batch, _residue_batch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

SLICE = "SHELFI_DOTP_SLICE_CTS"
CHUNK = "SHELFI_EVAL_CHUNK_MIB"
DEFAULT_SLICE_CTS = 256  # shelfi_internal.h Switches::dotp_slice_cts
FILL_GROUPS = 1024       # shelfi_internal.h kGramFillGroups

# id: (ring, towers, scale bits, first modulus bits, [level, ...])
CHAINS = {
    "n11": (1 << 11, 3, 52, 60, []),                 # single-block ring: geometry and the 60-bit fold
    "g11": (1 << 11, 3, 30, 45, []),                 # 45- / 31- / 30-bit towers: red_ok false
    "A": (1 << 12, 7, 52, 60, [7, 4, 1]),
    "C": (1 << 12, 12, 52, 60, [12, 5]),
    "D": (1 << 13, 6, 52, 60, [6]),
    "G": (1 << 12, 4, 30, 45, [4, 3, 2, 1]),         # red_ok false
    "n15": (1 << 15, 4, 52, 60, [4]),
    "E": (1 << 16, 6, 52, 60, [4]),
    "F": (1 << 17, 5, 52, 60, [5]),
}
CASES = [(cid, Ll) for cid, c in CHAINS.items() for Ll in c[4]]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _ones(P, Ll, N):
    return torch.ones((P, 2, Ll, N), dtype=torch.int64, device="cuda")


def _make(N, L, sb, fb, seed, batch=None):
    c = m.CKKS("ckks", batch or N // 2, sb, "", multDepth=L - 1, firstModBits=fb, ringDim=N, seed=seed, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    assert (inf["ring_dim"], inf["num_towers"]) == (N, L)
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    return dict(c=c, inf=inf, q=q, psi=psi, N=N, L=L, seed=seed)


@functools.lru_cache(maxsize=None)
def chain(cid):
    """One context per chain for the whole module: its key pair, and NO evaluation key."""
    N, L, sb, fb = CHAINS[cid][:4]
    return _make(N, L, sb, fb, 1600 + sum(ord(ch) for ch in cid))


def _rng(cid, Ll, salt):
    return np.random.default_rng([sum(ord(ch) for ch in cid), Ll, salt])


def _plain_batch(rng, q, K, Ll, N):
    """[K][Ll][N] residues, uniform below each tower's modulus."""
    return _residue_batch(rng, q, K, Ll, N)[:, 0].copy()


def _project(x, us, pts, how="separate"):
    """device.project into a buffer of ones.  how: the batches as separate allocations, as views of one stacked
    tensor, or the stacked tensor itself.  pts: [R][K][Ll][N]."""
    n, (K, _, Ll, N) = len(us), us[0].shape
    if how == "separate":
        ts = [_dev(u) for u in us]
        arg = ts
    else:
        stack = _dev(np.stack(us))
        ts = [stack[i] for i in range(n)]
        arg = ts if how == "views" else stack
    pd = _dev(pts)
    out = _ones(n * len(pts), Ll, N)
    assert D.project(x["c"], arg, pd, out=out) is out
    for t, u in zip(ts, us):
        assert np.array_equal(_u64(t), u)  # the inputs are read only
    assert np.array_equal(_u64(pd), pts)
    return _u64(out)


# ---------------------------------------------------------------- tile geometry ----
@functools.lru_cache(maxsize=None)
def _geometry():
    """16 uniform ciphertext batches and 16 plaintext batches of K = 3 at 2^11 / L3; the reference of the first
    five of each (the K = 2 reference of the 16 x 1 and 1 x 16 cases is their own)."""
    x = chain("n11")
    rng = _rng("n11", 3, 1)
    us = [_residue_batch(rng, x["q"], 3, 3, x["N"]) for _ in range(16)]
    pts = np.stack([_plain_batch(rng, x["q"], 3, 3, x["N"]) for _ in range(16)])
    ref = PJ.project_ref(us[:5], pts[:5], x["q"])
    ref.setflags(write=False)
    return us, pts, ref


def _geometry_ref(n, R):
    us, pts, ref = _geometry()
    return us[:n], pts[:R], ref[[c * 5 + r for c in range(n) for r in range(R)]]


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_every_tile_shape(n, R):
    x = chain("n11")
    us, pts, ref = _geometry_ref(n, R)
    got = _project(x, us, pts)
    assert got.shape == (n * R, 2, 3, x["N"])
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("n,R", [(16, 1), (1, 16)])
def test_sixteen_by_one(n, R):
    x = chain("n11")
    us, pts, _ = _geometry()
    us, pts = [u[:2] for u in us[:n]], np.ascontiguousarray(pts[:R, :2])
    assert np.array_equal(_project(x, us, pts), PJ.project_ref(us, pts, x["q"]))


@pytest.mark.parametrize("how", ["separate", "views", "stacked"])
def test_batches_given_three_ways(how):
    us, pts, ref = _geometry_ref(5, 3)
    assert np.array_equal(_project(chain("n11"), us, pts, how), ref)


def test_one_tensor_at_two_indices():
    x = chain("n11")
    us, pts, ref = _geometry_ref(5, 2)
    ts = [_dev(u) for u in us]
    out = _ones(10, 3, x["N"])
    got = _u64(D.project(x["c"], [ts[0], ts[1], ts[2], ts[1], ts[4]], _dev(pts), out=out))
    assert np.array_equal(got[6:8], got[2:4]) and np.array_equal(got[6:8], ref[2:4])
    keep = [0, 1, 2, 3, 4, 5, 8, 9]
    assert np.array_equal(got[keep], ref[keep])


def test_dot_plain_is_entry_zero_and_mult_plain_at_one():
    x = chain("n11")
    c = x["c"]
    us, pts, ref = _geometry_ref(1, 1)
    ct, pt = _dev(us[0]), _dev(pts[0])
    out = _ones(1, 3, x["N"])
    assert D.dot_plain(c, ct, pt, out=out) is out
    assert np.array_equal(_u64(out), ref[:1])
    assert torch.equal(D.project(c, [ct], pt), out) and torch.equal(D.project(c, ct[None], pt[None]), out)
    one = D.dot_plain(c, ct[:1], pt[:1])
    assert torch.equal(one, D.mult_plain(c, ct[:1], pt[:1]))
    assert np.array_equal(_u64(one), PR.mult_plain(us[0][:1], pts[0][:1], x["q"]))


# ----------------------------------------------------------- rings and chains ----
@pytest.mark.parametrize("cid,Ll", CASES, ids=str)
def test_rings_and_chains(cid, Ll):
    x = chain(cid)
    rng = _rng(cid, Ll, 2)
    R = 1 if cid == "F" else 2
    us = [_residue_batch(rng, x["q"], 2, Ll, x["N"]) for _ in range(2)]
    pts = np.stack([_plain_batch(rng, x["q"], 2, Ll, x["N"]) for _ in range(R)])
    got = _project(x, us, pts)
    assert got.shape == (2 * R, 2, Ll, x["N"])
    assert np.array_equal(got, PJ.project_ref(us, pts, x["q"]))


# ------------------------------------------------------------------ fold edges ----
@pytest.mark.parametrize("K", [127, 128, 129, 255, 256, 257, 511, 512, 513])
@pytest.mark.parametrize("cid", ["n11", "g11"])
def test_maximal_products_in_one_slice(cid, K, monkeypatch):
    x = chain(cid)
    Ll, N, q = x["L"], x["N"], x["q"]
    set_switch(monkeypatch, SLICE, "100000")
    full = _full_batch(q, K, Ll, N)
    out = _ones(1, Ll, N)
    got = _u64(D.project(x["c"], [_dev(full)], _dev(full[:, 0]), out=out))
    assert x["c"].dotp_slice_count() == 1
    for t in range(Ll):
        assert (got[0, :, t] == np.uint64(K % int(q[t]))).all(), t


@pytest.mark.parametrize("cid", ["n11", "g11"])
def test_one_maximal_learner_and_plaintext_among_uniform_ones(cid, monkeypatch):
    x = chain(cid)
    Ll, N, q, K = x["L"], x["N"], x["q"], 17
    set_switch(monkeypatch, SLICE, "100000")
    rng = _rng(cid, Ll, 3)
    us = [_residue_batch(rng, q, K, Ll, N), _full_batch(q, K, Ll, N), _residue_batch(rng, q, K, Ll, N)]
    pts = np.stack([_full_batch(q, K, Ll, N)[:, 0], _plain_batch(rng, q, K, Ll, N)])
    assert np.array_equal(_project(x, us, pts), PJ.project_ref(us, pts, q))
    assert x["c"].dotp_slice_count() == 1


# ---------------------------------------------------------------------- slices ----
def _tiles(n, R):
    """include/shelfi.h: 2 x 2 tiles, and the learners by four, two and one at R = 1."""
    return n // 4 + (n % 4) // 2 + n % 2 if R == 1 else -(-n // 2) * -(-R // 2)


def _slices(n, R, K, towers, N, cts, mib=2048):
    """include/shelfi.h: min(16, ceil(K / cts), ceil(1024 / workgroups a slice)), lowered until S C R ciphertexts
    fit the budget."""
    groups = _tiles(n, R) * towers * max(1, N // 512)
    S = min(16, -(-K // cts), -(-FILL_GROUPS // groups))
    while S > 1 and S * n * R * 2 * towers * N * 8 > mib << 20:
        S -= 1
    return S


def test_slices_do_not_change_a_bit(monkeypatch):
    x = chain("n11")
    c, N, K = x["c"], x["N"], 5
    rng = _rng("n11", 3, 4)
    us = [_residue_batch(rng, x["q"], K, 3, N)]
    pts = _plain_batch(rng, x["q"], K, 3, N)[None]
    ref = PJ.project_ref(us, pts, x["q"])
    set_switch(monkeypatch, SLICE, "1000")
    one = _project(x, us, pts)
    assert c.dotp_slice_count() == 1
    assert np.array_equal(one, ref)
    for val, slices in (("1", 5), ("2", 3), ("3", 2), (None, 1)):
        set_switch(monkeypatch, SLICE, val)
        assert np.array_equal(_project(x, us, pts), one), val
        assert c.dotp_slice_count() == slices == _slices(1, 1, K, 3, N, int(val or DEFAULT_SLICE_CTS)), val


def test_slices_are_capped_at_16_and_a_refusal_keeps_the_count(monkeypatch):
    x = chain("n11")
    c, N, K = x["c"], x["N"], 17
    rng = _rng("n11", 3, 5)
    us = [_residue_batch(rng, x["q"], K, 3, N)]
    pts = _plain_batch(rng, x["q"], K, 3, N)[None]
    set_switch(monkeypatch, SLICE, "1")
    assert np.array_equal(_project(x, us, pts), PJ.project_ref(us, pts, x["q"]))
    assert c.dotp_slice_count() == 16 == _slices(1, 1, K, 3, N, 1)  # 17 ciphertexts: one slice of two, fifteen of one
    t = _dev(us[0])
    with pytest.raises(ValueError, match="overlap"):
        D.project(c, [t], _dev(pts), out=t[3:4])
    assert c.dotp_slice_count() == 16


def test_the_scratch_budget_lowers_the_slice_count(monkeypatch):
    """2^11 / L3, K = 3, a ciphertext a slice: a ciphertext is 96 KiB.  Under a 1 MiB budget the 4 partial
    ciphertexts a slice of C = R = 2 fit twice (768 KiB), not three times, and the 16 of C = R = 4 (1.5 MiB) do
    not fit at all: one slice, no partials."""
    x = chain("n11")
    c, N = x["c"], x["N"]
    us, pts, _ = _geometry()
    set_switch(monkeypatch, SLICE, "1")
    for n, free, low in ((2, 3, 2), (4, 3, 1)):
        a, p = us[:n], pts[:n]
        set_switch(monkeypatch, CHUNK, None)
        whole = _project(x, a, p)
        assert c.dotp_slice_count() == free == _slices(n, n, 3, 3, N, 1)
        assert np.array_equal(whole, PJ.project_ref(a, p, x["q"]))
        set_switch(monkeypatch, CHUNK, "1")
        assert np.array_equal(_project(x, a, p), whole)
        assert c.dotp_slice_count() == low == _slices(n, n, 3, 3, N, 1, mib=1)


# ------------------------------------------------------------------------ keys ----
def test_no_key_of_any_kind_is_needed():
    """The module's contexts hold no evaluation key; a context that never had keys gives the same bits."""
    x = chain("n11")
    assert not x["c"].eval_key_info()["has_key"]
    bk = m.CKKS("ckks", 1024, 52, "", multDepth=2, firstModBits=60, ringDim=2048, seed=1, decodeNoise=False)
    assert not bk.info()["keys_loaded"] and bk.info()["moduli"] == x["inf"]["moduli"]
    us, pts, ref = _geometry_ref(3, 2)
    assert np.array_equal(_project(dict(c=bk), us, pts), ref)
    assert bk.dotp_slice_count() == 1
    assert not bk.info()["keys_loaded"]


# ----------------------------------------------------------------------- guards ----
def test_guards():
    x = chain("A")
    c, q, N, L = x["c"], x["q"], x["N"], x["L"]
    lib = _lib.load()
    rng = _rng("A", 4, 7)
    n, R, K, Ll = 3, 2, 3, 4
    P = n * R
    us = [_residue_batch(rng, q, K, Ll, N) for _ in range(n)]
    pts = np.stack([_plain_batch(rng, q, K, Ll, N) for _ in range(R)])
    ref = PJ.project_ref(us, pts, q)
    assert np.array_equal(_project(x, us, pts), ref)
    count = c.dotp_slice_count()
    mp_ref = PR.mult_plain(us[0][:1], pts[0][:1], q)
    # the inputs in one arena with room for an output behind them: an overlapping call stays inside it
    arena = torch.zeros((n * K + P, 2, Ll, N), dtype=torch.int64, device="cuda")
    for i, u in enumerate(us):
        arena[i * K:(i + 1) * K] = _dev(u)
    before = arena.clone()
    ctb = 2 * Ll * N * 8
    ptr = [arena.data_ptr() + i * K * ctb for i in range(n)]
    # the plaintexts with room for an output behind them as well
    parena = torch.zeros((R * K * Ll * N + P * 2 * Ll * N,), dtype=torch.int64, device="cuda")
    parena[:R * K * Ll * N] = _dev(pts).reshape(-1)
    pbefore = parena.clone()
    pp = parena.data_ptr()
    pd = parena[:R * K * Ll * N].view(R, K, Ll, N)
    out = _ones(P, Ll, N)
    po = out.data_ptr()
    # (buffers as large as the refused shapes would need: the call under test stays inside them)
    wide = torch.zeros((n * K + P + R * K, 2, L + 1, N), dtype=torch.int64, device="cuda")
    wct = 2 * (L + 1) * N * 8
    wptr = [wide.data_ptr() + i * K * wct for i in range(n)]
    many = torch.zeros((33, 1, 2, Ll, N), dtype=torch.int64, device="cuda")
    mpts = torch.zeros((33, 1, Ll, N), dtype=torch.int64, device="cuda")
    mout = torch.ones((33, 2, Ll, N), dtype=torch.int64, device="cuda")
    mptr = [many[i].data_ptr() for i in range(33)]

    def raw(ptrs, nb, pt, nr, Kc, towers, o):
        arr = None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)
        return lib.shelfi_dev_project(c._ctx, arr, nb, C.c_void_p(pt), nr, Kc, towers, C.c_void_p(o), None)

    def last():
        return lib.shelfi_last_error().decode()

    # C and R outside 1..32, by name
    assert raw(ptr, 0, pp, R, K, Ll, po) == _lib.SHELFI_ERR_ARG and "1..32 ciphertext" in last()
    assert raw(mptr, 33, mpts.data_ptr(), 1, 1, Ll, mout.data_ptr()) == _lib.SHELFI_ERR_ARG and "1..32 ciphertext" in last()
    assert raw(ptr, n, pp, 0, K, Ll, po) == _lib.SHELFI_ERR_ARG and "1..32 plaintext" in last()
    assert raw(mptr[:1], 1, mpts.data_ptr(), 33, 1, Ll, mout.data_ptr()) == _lib.SHELFI_ERR_ARG and "1..32 plaintext" in last()
    assert bool((mout == 1).all())
    refused = [
        lambda: raw(ptr, 0, pp, R, K, Ll, po),                               # C = 0
        lambda: raw(mptr, 33, mpts.data_ptr(), 1, 1, Ll, mout.data_ptr()),   # C = 33
        lambda: raw(ptr, n, pp, 0, K, Ll, po),                               # R = 0
        lambda: raw(mptr[:1], 1, mpts.data_ptr(), 33, 1, Ll, mout.data_ptr()),  # R = 33
        lambda: raw(ptr, n, pp, R, 0, Ll, po),                               # K = 0
        lambda: raw(ptr, n, pp, R, K, 0, po),                                # towers 0
        lambda: raw(wptr, n, wide.data_ptr() + (n * K + P) * wct, R, K, L + 1, wide.data_ptr() + n * K * wct),  # L + 1
        lambda: raw(None, n, pp, R, K, Ll, po),                              # NULL pointers
        lambda: raw([ptr[0], None, ptr[2]], n, pp, R, K, Ll, po),
        lambda: raw(ptr, n, None, R, K, Ll, po),
        lambda: raw(ptr, n, pp, R, K, Ll, None),
        lambda: raw(ptr, n, pp, R, K, Ll, ptr[0]),                           # out aliasing the first batch
        lambda: raw(ptr, n, pp, R, K, Ll, ptr[1]),                           # ... an inner one
        lambda: raw(ptr, n, pp, R, K, Ll, ptr[2] + 2 * ctb),                 # out overlapping the last batch by one ciphertext
        lambda: raw(ptr, n, pp, R, K, Ll, ptr[2] + ctb + ctb // 2),          # ... at a shift inside it
        lambda: raw([ptr[1], ptr[2], ptr[2]], n, pp, R, K, Ll, ptr[0] + ctb),  # out's tail reaching into a batch given twice
        lambda: raw(ptr, n, pp, R, K, Ll, pp),                               # out aliasing the plaintexts
        lambda: raw(ptr, n, pp, R, K, Ll, pp + (R * K * Ll * N - 2) * 8),    # ... overlapping their last two words
    ]
    for i, call in enumerate(refused):
        assert call() == _lib.SHELFI_ERR_ARG, i
        assert c.dotp_slice_count() == count, i
        assert torch.equal(out, _ones(P, Ll, N)) and torch.equal(arena, before) and torch.equal(parena, pbefore), i
        assert not bool(wide.any()) and bool((mout == 1).all()), i
        assert np.array_equal(_u64(D.project(c, [arena[j * K:(j + 1) * K] for j in range(n)], pd)), ref), i
        assert np.array_equal(_u64(D.mult_plain(c, arena[:1], pd[0, :1])), mp_ref), i
    # the same through device.project
    ts = [arena[i * K:(i + 1) * K] for i in range(n)]
    for call in (lambda: D.project(c, [], pd),
                 lambda: D.project(c, [many[i] for i in range(33)], mpts[:1]),
                 lambda: D.project(c, [many[0]], mpts),
                 lambda: D.project(c, ts, pd[:0]),
                 lambda: D.project(c, [t[:0] for t in ts], pd[:, :0]),
                 lambda: D.project(c, ts, pd, out=arena[:P]),
                 lambda: D.project(c, ts, pd, out=arena[n * K - 1:n * K - 1 + P]),
                 lambda: D.project(c, [ts[0], ts[1][:2]], pd),
                 lambda: D.project(c, ts, pd[:, :2].contiguous()),
                 lambda: D.project(c, ts, pd[:, :, :3].contiguous()),
                 lambda: D.project(c, ts, pd[:, :2]),
                 lambda: D.project(c, ts, pd.cpu()),
                 lambda: D.project(c, ts, pd, out=_ones(P - 1, Ll, N)),
                 lambda: D.project(c, ts, pd, out=_ones(P, Ll - 1, N)),
                 lambda: D.project(c, arena[:n * K].view(n, K, 2, Ll, N)[:, :, :1], pd),
                 lambda: D.dot_plain(c, ts[0], pd),
                 lambda: D.project(c, [wide[:K], wide[K:2 * K]], pd)):
        with pytest.raises(ValueError):
            call()
        assert c.dotp_slice_count() == count
    assert torch.equal(arena, before) and torch.equal(parena, pbefore)
    assert np.array_equal(_u64(D.project(c, ts, pd, out=arena[n * K:])), ref)


# ---------------------------------------------------------------------- meaning ----
def test_project_rescale_eval_sum_decrypts_to_the_projections():
    """2^12 / L3, C = 3 learners of K = 4 ciphertexts of 2048 slots against R = 2 known vectors encoded at scale
    q_2: after ModReduce and EvalSum over the slots, slot 0 of entry c R + r holds <x_c, g_r> over all 8192
    values (test_gpu_dot.py's end-to-end bound).  Measured: 3.5e-10."""
    x = _make(1 << 12, 3, 52, 60, 1661)
    c, q, N, inf = x["c"], x["q"], x["N"], x["inf"]
    c.evalSumKeyGen()
    S, K, n, R = inf["batch"], 4, 3, 2
    rng = np.random.default_rng(10)
    xs, gs = rng.uniform(-1, 1, (n, K * S)), rng.uniform(-1, 1, (R, K * S))
    us = [D.encrypt(c, torch.tensor(v, dtype=torch.float64, device="cuda")) for v in xs]
    pts = torch.stack([D.encode(c, torch.tensor(g, dtype=torch.float64, device="cuda"), towers=3, scale=float(q[2]))
                       for g in gs])
    assert us[0].shape == (K, 2, 3, N) and pts.shape == (R, K, 3, N)
    out = _ones(n * R, 3, N)
    prj = D.project(c, us, pts, out=out)
    tot = D.eval_sum(c, D.rescale(c, prj), S)
    dec = D.decrypt(c, tot, n * R * S, inf["delta"]).cpu().numpy().reshape(n * R, S)
    exp = np.array([np.dot(xs[i], gs[r]) for i in range(n) for r in range(R)])
    err = float(np.abs(dec[:, 0] - exp).max())
    print("projections: max error %.3g" % err)
    assert err < 1e-6


def test_pack_slots_opens_a_gram_matrix_with_one_decrypt():
    """2^12 / L4, C = 4 learners of K = 2 ciphertexts, inputs U(-0.1, 0.1) (every Gram entry below 41 < 2^7):
    gram (4 towers, scale delta^2) -> rescale (3 towers, delta^2 / q_3) -> eval_sum -> pack_slots (2 towers, the
    same scale) -> decrypt of ONE ciphertext, against the P = 10 separate decrypts and numpy; and the packed
    ciphertext bit for bit against pack_ref on the same inputs.  Measured: 4.6e-10 against the
    separate decrypts, 4.4e-10 against numpy, at most 1.1e-12 in the other slots."""
    x = _make(1 << 12, 4, 52, 60, 1662)
    c, q, psi, N, inf = x["c"], x["q"], x["psi"], x["N"], x["inf"]
    c.evalMultKeyGen()
    c.evalSumKeyGen()
    S, K, n = inf["batch"], 2, 4
    xs = np.random.default_rng(11).uniform(-0.1, 0.1, (n, K * S))
    us = [D.encrypt(c, torch.tensor(v, dtype=torch.float64, device="cuda")) for v in xs]
    pairs = D.gram_pairs(n)
    P = len(pairs)
    scale = inf["delta"] * inf["delta"] / float(q[3])
    tot = D.eval_sum(c, D.rescale(c, D.gram(c, us)), S)
    assert tot.shape == (P, 2, 3, N)
    out = torch.ones((1, 2, 2, N), dtype=torch.int64, device="cuda")
    packed = D.pack_slots(c, tot, out=out)
    assert packed is out
    one = D.decrypt(c, packed, S, scale).cpu().numpy()
    each = D.decrypt(c, tot, P * S, scale).cpu().numpy().reshape(P, S)[:, 0]
    exp = np.array([np.dot(xs[i], xs[j]) for i, j in pairs])
    e_each, e_np = float(np.abs(one[:P] - each).max()), float(np.abs(one[:P] - exp).max())
    rest = float(np.abs(one[P:]).max())
    print("pack_slots: against the separate decrypts %.3g, against numpy %.3g, the other slots %.3g" % (e_each, e_np, rest))
    assert e_each < 1e-6 and e_np < 1e-6
    assert np.array_equal(_u64(packed), PJ.pack_ref(_u64(tot), S, q, psi))
    assert torch.equal(D.pack_slots(c, tot), packed)  # (the cached one-hot plaintexts)


def test_pack_slots_shapes():
    """P = 1 and P = batch are accepted (a context of 8 slots, no keys: pack_slots needs none), bit for bit
    pack_ref's; P = batch + 1 and one tower are refused."""
    ck = m.CKKS("ckks", 8, 52, "", multDepth=1, firstModBits=60, ringDim=2048, seed=2, decodeNoise=False)
    inf = ck.info()
    assert inf["batch"] == 8 and inf["num_towers"] == 2
    q, psi, N = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64), 2048
    cts = _residue_batch(np.random.default_rng(12), q, 9, 2, N)
    for P in (1, 8):
        out = torch.ones((1, 2, 1, N), dtype=torch.int64, device="cuda")
        assert np.array_equal(_u64(D.pack_slots(ck, _dev(cts[:P]), out=out)), PJ.pack_ref(cts[:P], 8, q, psi)), P
    with pytest.raises(ValueError, match="batch"):
        D.pack_slots(ck, _dev(cts))
    with pytest.raises(ValueError, match="2 towers"):
        D.pack_slots(ck, _dev(cts[:2, :, :1]))


# ------------------------------------------------------------------- neighbours ----
def test_neighbours_give_the_same_bits_around_a_project(monkeypatch):
    x = _make(1 << 13, 3, 52, 60, 1663)
    c, q, N = x["c"], x["q"], x["N"]
    c.evalMultKeyGen()
    rng = np.random.default_rng(13)
    a, b = (_dev(_residue_batch(rng, q, 2, 3, N)) for _ in range(2))
    pt = _dev(_plain_batch(rng, q, 2, 3, N))

    def neighbours():
        return D.mult_plain(c, a, pt), D.dot(c, a, b), D.gram(c, [a, b]), D.mult(c, a, b)

    before = neighbours()
    big = _dev(np.stack([_residue_batch(rng, q, 4, 3, N) for _ in range(5)]))
    bpts = _dev(np.stack([_plain_batch(rng, q, 4, 3, N) for _ in range(3)]))
    set_switch(monkeypatch, SLICE, "1")  # four slices: the partial sums go through the context's scratch
    D.project(c, big, bpts)
    assert c.dotp_slice_count() == 4
    D.project(c, [big[4], big[0], big[4]], bpts[:1])
    for u, v in zip(before, neighbours()):
        assert torch.equal(u, v)
