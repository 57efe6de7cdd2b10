"""The aggregation kernels (fhe-fed_amd/csrc/wavg.hip) at the limits of their carry-free limb sums
and at the edges of their learner groups, bit-exact against the oracle.

Inputs come from tests/wavg_cases.py: in one target tower every learner holds xmax(q_t) at planted
positions and carries a float32 weight whose W mod q_t has both limbs at their largest, so a full
group of learners fills S0 / s00 (and, at a 60-bit tower, Sm / s01 / s10 / s11) to within 2^-13 of
2^64 (tests/test_wavg_cases.py derives that on the CPU); learner counts sit on the group edges
(8 and 16 learners, and the launches of 16), every packed width class runs, and the 60-bit class
is reached by towers of 58, 59 and 60 bits.  Every input is canonical and every weight is accepted
by the library: nothing here overflows unless a group is widened or a slice is read from the wrong
place.

Each case has two weight vectors, run back to back on the same arena (the device weight ring):
w_sat, all learners at the saturating weight -- the vector a widened group wraps on -- and w_mix,
the same with a zero and a positive weight among them."""
import os
import types

import numpy as np
import pytest

import arena_layout as AL
import oracle as O
import wavg_cases as WC
from conftest import set_switch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

EDGE_C = (1, 7, 8, 9, 15, 16, 17)
MORE_C = (24, 25, 32, 33)          # a third group of 8, the second and third launch of 16
POINTER_C = (1, 8, 9, 15, 16, 17, 32, 33)
BYTES_C = (8, 9, 16, 17)
# (SHELFI_PACK_KERNEL, SHELFI_PACK_UNROLL, SHELFI_PACK_WAVES)
PACK_SWITCHES = [(None, None, None), ("r3", None, None), ("v4", "1", None), ("v4", "2", None), ("v4", "4", None),
                 ("v4", "8", None), (None, None, "2"), (None, None, "8"), ("v4", None, "2"), ("v4", None, "8")]


def _K(C):
    """Ciphertexts per learner: 2 where the sub-range k0 = 1 is taken as well."""
    return 2 if C in (9, 17) else 1


def _has60(q):
    return any(WC.width(x) == 60 for x in q)


def _rows(rows):
    """Parametrise a test over parameter rows through the module-scoped fixture rc, so all tests of
    a row run together and share its context and references."""
    return pytest.mark.parametrize("rc", rows, indirect=True, ids=["s%d-f%d-d%d" % r for r in rows])


# the rows of the packed-output, stacked-sum and modq tests: the reference chain and the chain with
# 58-, 59- and 60-bit towers (the first two rows, so both parametrisations index them alike)
STACK_ROWS = WC.PARAM_ROWS[:2]
assert STACK_ROWS == [(52, 60, 1), (58, 60, 3)]


@pytest.fixture(scope="module")
def rc(request, tmp_path_factory):
    """One parameter row: its context at ring 1024 and the row's cases with their references (each
    computed once, shared by the tests of the row, never written to)."""
    scale, first, depth = request.param
    d = str(tmp_path_factory.mktemp("wl_%d_%d_%d" % request.param)) + os.sep
    ck = m.CKKS("ckks", 512, scale, d, multDepth=depth, firstModBits=first, ringDim=WC.RING, seed=11,
                decodeNoise=False)
    assert ck.genCryptoContextAndKeyGen() == 1
    inf = ck.info()
    q = np.array(inf["moduli"], np.uint64)
    qo, _ = O.params_generate(WC.RING, depth + 1, scale, first)
    assert inf["ring_dim"] == WC.RING and np.array_equal(q, qo)
    r = types.SimpleNamespace(row=request.param, ck=ck, q=q, L=len(q), N=WC.RING, delta=inf["delta"], cases={})
    yield r
    r.cases.clear()


def _case(rc, t, C):
    """build_case + oracle.wavg for both weight vectors; the oracle is held to the Python-int sum at
    the planted and sampled positions here, so a kernel equal to it is equal to both."""
    key = (t, C)
    if key not in rc.cases:
        case = WC.build_case(rc.q, rc.delta, C, t, _K(C))
        case.refs = []
        for w in (case.w_sat, case.w_mix):
            ref = O.wavg(case.cts, w, rc.q, rc.delta)
            exact = WC.wavg_exact(case.cts, [WC.weight_int(x, rc.delta) for x in w], rc.q, case.positions)
            assert [int(ref[p]) for p in case.positions] == exact
            ref.setflags(write=False)
            case.refs.append(ref)
        rc.cases[key] = case
    return rc.cases[key]


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _dev(a):
    return torch.from_numpy(a.view(np.int64)).cuda()


def _where(got, ref):
    bad = np.argwhere(got != ref)
    return "%d residues differ, first (k, poly, tower, j) = %s" % (len(bad), bad[:4].tolist())


def _eq(got, ref, *ctx):
    assert np.array_equal(got, ref), (ctx, _where(got, ref))


def _set_pack(monkeypatch, kern, unroll, waves):
    set_switch(monkeypatch, "SHELFI_PACK_KERNEL", kern)
    set_switch(monkeypatch, "SHELFI_PACK_UNROLL", unroll)
    set_switch(monkeypatch, "SHELFI_PACK_WAVES", waves)


def _packed_arena(rc, case):
    ar = D.Arena(rc.ck, case.C, case.K, layout="packed")
    for c in range(case.C):  # placement alternates by learner: device tensor, host blob
        ar.put(c, m.blob_pack(rc.ck, case.cts[c]) if c % 2 else _dev(case.cts[c]))
    return ar


@_rows(WC.PARAM_ROWS)
def test_packed_arena_group_edges(rc, monkeypatch):
    """wavg_packed (v4, every unroll and wave count) and wavg_packed_r3 on the packed arena: learner
    counts on both sides of every group edge, each tower of the row saturated in turn, both weight
    vectors back to back, the sub-range k0 = 1 where K = 2."""
    counts = EDGE_C + (MORE_C if _has60(rc.q) or rc.row == (52, 60, 1) else ())
    for t in range(rc.L):
        for C in counts:
            case = _case(rc, t, C)
            ar = _packed_arena(rc, case)
            for sw in PACK_SWITCHES:
                _set_pack(monkeypatch, *sw)
                for w, ref in ((case.w_sat, case.refs[0]), (case.w_mix, case.refs[1])):
                    _eq(_host(ar.wavg(w)), ref, rc.row, t, C, sw)
                    if case.K > 1 and sw[2] is None:
                        _eq(_host(ar.wavg(w, k0=1)), ref[1:], rc.row, t, C, sw, "k0=1")
            _set_pack(monkeypatch, None, None, None)
            # the planted and sampled positions against the Python-int sum, directly
            got = _host(ar.wavg(case.w_sat))
            Ws = [WC.weight_int(x, rc.delta) for x in case.w_sat]
            assert [int(got[p]) for p in case.positions] == WC.wavg_exact(case.cts, Ws, rc.q, case.positions)
            ar.release()


@_rows(WC.PARAM_ROWS)
def test_pointer_kernel_group_edges(rc, monkeypatch):
    """wavg_kernel over separate uint64 batches (D.wavg): both rows-per-block classes, one launch of
    up to 16 learners and the accumulating launches at 17, 32 and 33."""
    for t in range(rc.L):
        for C in POINTER_C:
            case = _case(rc, t, C)
            dev = [_dev(c) for c in case.cts]
            for rows in (None, "1", "2"):
                set_switch(monkeypatch, "SHELFI_WAVG_ROWS", rows)
                for w, ref in ((case.w_sat, case.refs[0]), (case.w_mix, case.refs[1])):
                    _eq(_host(D.wavg(rc.ck, dev, w)), ref, rc.row, t, C, rows)
            set_switch(monkeypatch, "SHELFI_WAVG_ROWS", None)


def _packed_blob(rc, ct):
    """A version-2 (packed wire) blob of these residues: the uint64 blob's header with the version
    field set to 2 and the payload packed by tests/arena_layout.py."""
    hdr = m._lib.load().shelfi_blob_header_bytes()
    b = bytearray(m.blob_pack(rc.ck, ct)[:hdr])
    b[4:6] = (2).to_bytes(2, "little")
    return bytes(b) + AL.pack_one(ct, rc.q, rc.N).tobytes()


@_rows(WC.PARAM_ROWS)
def test_bytes_api_group_edges(rc):
    """computeWeightedAverage on blobs of the same residues (the residue-checking instantiation of
    wavg_kernel), in the uint64 and the packed wire format; on (52, 60, 1) also the uint64 arena."""
    ck = rc.ck
    try:
        for t in range(rc.L):
            for C in BYTES_C:
                case = _case(rc, t, C)
                ck.set_wire_format("shelfi")
                blobs = [m.blob_pack(ck, c) for c in case.cts]
                for w, ref in ((case.w_sat, case.refs[0]), (case.w_mix, case.refs[1])):
                    agg = ck.computeWeightedAverage(blobs, w)
                    _eq(m.blob_residues(agg, rc.N, rc.L), ref, rc.row, t, C, "shelfi")
                ck.set_wire_format("packed")
                blobs = [_packed_blob(rc, c) for c in case.cts]
                for w, ref in ((case.w_sat, case.refs[0]), (case.w_mix, case.refs[1])):
                    agg = ck.computeWeightedAverage(blobs, w)
                    assert m.blob_info(agg)["format"] == "packed"
                    _eq(m.blob_residues(agg, rc.N, rc.L, ckks=ck), ref, rc.row, t, C, "packed")
                if rc.row == (52, 60, 1):
                    ar = D.Arena(ck, C, case.K, layout="uint64")
                    for c in range(C):
                        ar.put(c, blobs[c] if c % 2 else _dev(case.cts[c]))
                    for w, ref in ((case.w_sat, case.refs[0]), (case.w_mix, case.refs[1])):
                        _eq(_host(ar.wavg(w)), ref, rc.row, t, C, "uint64 arena")
    finally:
        ck.set_wire_format("shelfi")


@_rows(STACK_ROWS)
def test_packed_output_and_stacked_sum_limits(rc):
    """Arena.wavg_packed on the saturating cases, read back through sum_packed(G = 1), equals
    Arena.wavg; sum_packed of G stacked packed batches (every target-tower residue at q_t - 1, the
    edge residues in the other towers, a gap between the batches) equals their exact mod-q sum.  G
    runs over the group edges 8, 9 and 16; sum_packed takes at most 16 batches, and 17 is refused."""
    ck = rc.ck
    for t in range(rc.L):
        for C in BYTES_C:
            case = _case(rc, t, C)
            ar = _packed_arena(rc, case)
            pw = D.packed_words(ck, case.K)
            for w, ref in ((case.w_sat, case.refs[0]), (case.w_mix, case.refs[1])):
                packed = ar.wavg_packed(w)
                assert packed.numel() == pw
                _eq(_host(D.sum_packed(ck, packed, 1, case.K, pw)), ref, rc.row, t, C, "packed out")
                _eq(_host(ar.wavg(w)), ref, rc.row, t, C)
            ar.release()
        K = 1
        pw, stride = D.packed_words(ck, K), D.packed_words(ck, K) + 40
        batches = []
        for g in range(17):
            a = np.empty((K, 2, rc.L, rc.N), np.uint64)
            for u in range(rc.L):
                e = np.array(WC.edge_residues(int(rc.q[u])), np.uint64)
                a[:, :, u, :] = e[(np.arange(rc.N) + g) % len(e)]
            a[:, :, t, :] = int(rc.q[t]) - 1
            batches.append(a)
        stk = torch.zeros(17 * stride, dtype=torch.int64, device="cuda")
        for g, a in enumerate(batches):
            words = torch.from_numpy(AL.pack_one(a, rc.q, rc.N).view(np.int64))
            assert words.numel() == pw
            stk[g * stride:g * stride + pw] = words.cuda()
        for G in (8, 9, 16):
            exact = np.empty_like(batches[0])
            for u in range(rc.L):  # Python ints (object dtype): no 64-bit wrap in the reference
                s = sum(b[:, :, u, :].astype(object) for b in batches[:G]) % int(rc.q[u])
                exact[:, :, u, :] = s.astype(np.uint64)
            _eq(_host(D.sum_packed(ck, stk, G, K, stride)), exact, rc.row, t, G, "stacked")
        with pytest.raises(ValueError, match="1..16"):
            D.sum_packed(ck, stk, 17, K, stride)


@_rows(STACK_ROWS)
def test_modq_at_its_limit(rc):
    """D.modq at its documented limit: a uint64 sum of 15 partials, all q_t - 1 in the saturated
    tower (15 (q_t - 1) < 2^64 for q_t < 2^60) and random elsewhere, folds to the exact value."""
    rng = np.random.default_rng(15)
    for t in range(rc.L):
        parts = []
        for _ in range(15):
            a = np.empty((2, 2, rc.L, rc.N), np.uint64)
            for u in range(rc.L):
                a[:, :, u, :] = rng.integers(0, int(rc.q[u]), (2, 2, rc.N), dtype=np.uint64)
            a[:, :, t, :] = int(rc.q[t]) - 1
            parts.append(a)
        s = np.zeros_like(parts[0])
        for a in parts:
            s += a
        assert int(s[0, 0, t, 0]) == 15 * (int(rc.q[t]) - 1)  # no wrap in the collective's sum
        dev = _dev(s.copy())
        D.modq(rc.ck, dev)
        exact = np.empty_like(s)
        for u in range(rc.L):
            exact[:, :, u, :] = (sum(a[:, :, u, :].astype(object) for a in parts) % int(rc.q[u])).astype(np.uint64)
        _eq(_host(dev), exact, rc.row, t, "modq")
