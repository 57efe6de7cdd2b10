"""The multiparty key calls of threshold CKKS (multikey.hip, the three shelfi_multi_* entry
points, shelfi_multiparty_keygen) at the places tests/test_gpu_multikey.py leaves alone: planted previous and
joint keys, both lanes of the word pairs the key add reads, the b | a seam, every (vector, digit, tower) of
the device range checks with values at, just above and far above the modulus, the ends of the rotation index
range, a sparse-packing context (batch = N / 8), the (3, 4, 4) and 30-bit chains end to end, joint keys below
the top level, the refusal contract of the C entry points, and the threshold key chain over planted keys.

Everything is bit-exact against tests/multikey_ref.py (held to its meaning by tests/test_multikey_ref.py),
tests/rotation_ref.py and the oracle.  The sweeps take their references from MK.share_terms / MK.round2_terms,
which do a call's NTTs once; tests/test_multikey_ref.py holds those equal to MK.share / MK.round2, and each
sweep here checks its unplanted key against MK.share / MK.round2 itself.  2^11 / L3 runs every sweep whole;
the 2^12 chains run the corners (every digit, the first and the last tower, all four lanes), each word refused
on its own and q_t - 1 accepted at all of them in one call.

A planted word equal to its modulus q_t must be refused and the same word at q_t - 1 accepted: the two
together pin the modulus the kernel compares with at that word, so a wrong tower index shows wherever two
neighbouring towers differ (every seam of these chains: 60 | 52 | 53 | 60 bits, 45 | 31 | 30 bits).

Value tolerances: 1e-6 at a 52-bit scale (tests/test_gpu_multikey.py), max(1e-7, 2^(18 - scale bits)) at a
30-bit scale (tests/test_gpu_f4.py, tests/test_gpu_threshold.py).  The oracle's own error on the 30-bit case's
inputs (2^12 / L4, three parties, the seeds below) is 1.47e-4 after mult and rescale, 1.47e-4 after the
rotation and 2.32e-4 after eval_sum(4), all below 2^-12 = 2.44e-4, so the rule stands as it is."""
import contextlib
import functools

import numpy as np
import pytest

import multikey_ref as MK
import oracle as O
import rotation_ref as R
from f4_cases import _relin_defect

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

import test_gpu_multikey as G  # noqa: E402  (the shape table, parties(), joint_keys())

SHAPES = G.SHAPES
SPARSE = (1 << 12, 3, 52, 60)  # n12_sparse: batch = N / 8
PLANT_SHAPES = ("n11_L3", "n12_L4_30bit", "n12_L12", "n13_L3")
U64_MAX = (1 << 64) - 1
_u64 = G._u64


def _new_sparse(seed):
    N, L, sb, fb = SPARSE
    return m.CKKS("ckks", N // 8, sb, "", multDepth=L - 1, firstModBits=fb, ringDim=N, seed=seed, decodeNoise=False)


@functools.lru_cache(maxsize=None)
def _sparse_parties():
    """G.parties for the sparse-packing context: two parties after the threshold key chain."""
    N, L = SPARSE[:2]
    seeds = [3900, 3901]
    cs = [_new_sparse(s) for s in seeds]
    assert cs[0].genCryptoContextAndKeyGen() == 1
    keys = [cs[0].get_keys()]
    cs[1].multipartyKeyGen(keys[0][0])
    keys.append(cs[1].get_keys())
    pk = keys[-1][0]
    for c, (_, sk) in zip(cs, keys):
        c.set_keys(pk, sk)
        c.set_threshold_noise(0.0)
    inf = cs[0].info()
    assert (inf["ring_dim"], inf["num_towers"], inf["batch"]) == (N, L, N // 8)
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    dn, al, p, _ = O.special_primes(N, q)
    sks = [k[1] for k in keys]
    return dict(cs=cs, seeds=seeds, sks=sks, pk=pk, q=q, psi=psi, N=N, L=L, S=inf["batch"], d=inf["delta"], dn=dn,
                al=al, kP=len(p), mods=MK.ext_moduli(N, q), sk_sum=MK.sk_sum(sks, q), shape=(2, dn, L + len(p), N))


def X(sid, Pn=2):
    return _sparse_parties() if sid == "n12_sparse" else G.parties(sid, Pn)


def _uniform(x, *salt):
    return MK.uniform_key(np.random.default_rng(list(salt) + [x["N"]]), x["mods"], x["dn"], x["N"])


def _full(x):
    return MK.full_key(x["mods"], x["dn"], x["N"])


@contextlib.contextmanager
def plant(key, at, val):
    """key[at] = val for the block, the old word back after it."""
    old = key[at]
    key[at] = np.uint64(val)
    try:
        yield key
    finally:
        key[at] = old


def positions(x, js=None, ts=None, words=None):
    """(vector, digit, tower, word) of a sweep: everything, both lanes at both ends of a tower."""
    _, dn, T, N = x["shape"]
    return [(v, j, t, w) for v in range(2) for j in (range(dn) if js is None else js)
            for t in (range(T) if ts is None else ts) for w in ((0, 1, N - 2, N - 1) if words is None else words)]


def corners(x):
    """The thinned sweep of the larger shapes: every digit, the first and the last tower, every lane."""
    return positions(x, ts=(0, x["shape"][2] - 1))


@contextlib.contextmanager
def plant_all(key, places, val_of):
    """plant() at every place at once, val_of(tower) there."""
    with contextlib.ExitStack() as st:
        for pos in places:
            st.enter_context(plant(key, pos, val_of(pos[2])))
        yield key


def bad_values(x, t):
    """Non-canonical words for tower t: just above the modulus, the top bit, all ones, and -- in a tower
    narrower than tower 0 -- tower 0's largest residue."""
    mods = [int(v) for v in x["mods"]]
    vals = [mods[t] + 1, 1 << 63, U64_MAX]
    if mods[0] - 1 >= mods[t]:
        vals.append(mods[0] - 1)
    return vals


def value_places(x):
    """An even and an odd word of a 52-bit tower of Q and of a tower of P."""
    L, N = x["L"], x["N"]
    assert int(x["mods"][1]) < int(x["mods"][0])
    return [(1, N // 2), (1, N // 2 + 1), (L, 6), (L, 7)]


def refused(call, what="residue"):
    with pytest.raises(ValueError, match=what):
        call()


# ----------------------------------------------- A. follower shares over planted keys ----
def _planted_prevs(x):
    u, f, z = _uniform(x, 1), _full(x), np.zeros(x["shape"], np.uint64)
    a_uni_b_full = u.copy()
    a_uni_b_full[0] = f[0]
    digit0 = z.copy()
    digit0[1, 0] = f[1, 0]
    return {"full": f, "zero": z, "uniform": u, "a_uniform_b_full": a_uni_b_full, "a_full_in_digit_0": digit0}


@pytest.mark.parametrize("rk", ["0", "1", "-(S-1)"])
@pytest.mark.parametrize("sid", PLANT_SHAPES)
def test_follower_share_over_planted_prev(sid, rk):
    x = X(sid)
    c, seed, sk, q, psi = x["cs"][1], x["seeds"][1], x["sks"][1], x["q"], x["psi"]
    r = {"0": 0, "1": 1, "-(S-1)": -(x["S"] - 1)}[rk]
    terms = MK.share_terms(seed, sk, q, psi, r)
    other_b = _uniform(x, 2)[0]
    errs = []
    for name, prev in _planted_prevs(x).items():
        out = c.multiKeySwitchGen(prev, r)
        assert np.array_equal(out[1], prev[1]), name
        assert np.array_equal(out, MK.share_from_terms(terms, prev)), name
        if name in ("uniform", "a_full_in_digit_0"):
            assert np.array_equal(out, MK.share(seed, sk, q, psi, r, prev)), name
        twin = prev.copy()
        twin[0] = other_b  # prev's b-vector is range-checked and otherwise ignored
        assert np.array_equal(c.multiKeySwitchGen(twin, r), out), name
        e = MK.switch_key_error(out, r, sk, q, psi)
        assert (e == e[:, :1]).all() and 0 < np.abs(e).max() < MK.B_ERR, name
        errs.append(e[:, 0])
    for e in errs[1:]:  # the party's own error, whatever it is handed
        assert np.array_equal(e, errs[0])


# ----------------------------------------------------- B. rotation-share indices ----
def _index(x, rk):
    S = x["S"]
    return {"S-1": S - 1, "-(S-1)": -(S - 1), "S/2": S // 2, "-1": -1, "2": 2, "1": 1}[rk]


INDEX_CASES = ([(sid, rk) for sid in ("n11_L3", "n12_L12") for rk in ("S-1", "-(S-1)", "S/2", "-1", "2")]
               + [("n12_sparse", rk) for rk in ("1", "S-1", "-(S-1)")])


@pytest.mark.parametrize("sid,rk", INDEX_CASES, ids=str)
def test_rotation_share_indices(sid, rk):
    x = X(sid)
    (c0, c1), (s0, s1), (sk0, sk1) = x["cs"], x["seeds"], x["sks"]
    q, psi, r = x["q"], x["psi"], _index(x, rk)
    lead = c0.multiKeySwitchGen(None, r)
    assert np.array_equal(lead, MK.share(s0, sk0, q, psi, r))
    foll = c1.multiKeySwitchGen(lead, r)
    assert np.array_equal(foll, MK.share(s1, sk1, q, psi, r, lead))


def test_sparse_index_bound_is_the_batch():
    x = X("n12_sparse")
    S = x["S"]
    assert S == x["N"] // 8
    for c in x["cs"]:
        for r in (S, -S):
            with pytest.raises(ValueError, match="batch"):
                c.multiKeySwitchGen(None, r)
    prev = x["cs"][0].multiKeySwitchGen(None, S - 1)
    for r in (S, -S):
        with pytest.raises(ValueError, match="batch"):
            x["cs"][1].multiKeySwitchGen(prev, r)


@pytest.mark.parametrize("sid", ["n11_L3", "n12_sparse"])
def test_shares_of_different_indices_share_nothing(sid):
    """Under one seed the shares of 0 and of the indices of the sweep draw their own a and their own error: no
    a-row and no error row appears twice (test_share_streams_are_their_own's check, over all pairs).  The
    streams are named by the Galois element, and 5 has order N / 2 mod 2N: at a full batch S - 1 and -1 (and
    -(S - 1) and 1) are one rotation and give one share, bit for bit; at batch N / 8 they are four."""
    x = X(sid)
    c, sk, q, psi, S, N = x["cs"][0], x["sks"][0], x["q"], x["psi"], x["S"], x["N"]
    idx = [0, 1, 2, -1, S // 2, S - 1, -(S - 1)]
    by_g = {}
    for r in idx:
        by_g.setdefault(1 if r == 0 else R.galois(N, r), []).append(r)
    assert len(by_g) == (5 if S == N // 2 else 7)
    keys = {r: c.multiKeySwitchGen(None, r) for r in idx}
    for same in by_g.values():
        for r in same[1:]:
            assert np.array_equal(keys[r], keys[same[0]]), same
    reps = [same[0] for same in by_g.values()]
    errs = [MK.switch_key_error(keys[r], r, sk, q, psi)[:, 0] for r in reps]
    a_rows = [row.tobytes() for r in reps for row in keys[r][1].reshape(-1, N)]
    e_rows = [row.tobytes() for e in errs for row in e]
    assert len(set(a_rows)) == len(a_rows) == len(reps) * x["dn"] * x["shape"][2]
    assert len(set(e_rows)) == len(e_rows) == len(reps) * x["dn"]
    for i in range(len(reps)):  # and pair by pair, row by row, as the idiom has it
        for j in range(i + 1, len(reps)):
            assert not (keys[reps[i]][1] == keys[reps[j]][1]).all(axis=-1).any()
            assert not (errs[i] == errs[j]).all(axis=-1).any()


def test_positive_index_with_a_galois_element_above_2_16_at_n17():
    x = X("n17_L2")
    N, q, psi = x["N"], x["q"], x["psi"]
    r = MK.first_index_with_galois_above(N, 1 << 17)
    assert 0 < r < x["S"] and pow(5, r, 2 * N) > 1 << 17
    assert all(pow(5, k, 2 * N) <= 1 << 17 for k in range(1, r))
    lead = x["cs"][0].multiKeySwitchGen(None, r)
    assert np.array_equal(lead, MK.share(x["seeds"][0], x["sks"][0], q, psi, r))
    foll = x["cs"][1].multiKeySwitchGen(lead, r)
    assert np.array_equal(foll, MK.share(x["seeds"][1], x["sks"][1], q, psi, r, lead))


def _server(x, make, final=None, rot=None):
    """A context with the joint public key and no secret."""
    server = make(4242)
    server.set_keys(x["pk"], np.zeros((x["L"], x["N"]), np.uint64))
    if final is not None:
        server.set_eval_key(final)
    for r, key in (rot or {}).items():
        server.set_rotation_key(r, key)
    return server


def test_sparse_joint_rotation_on_a_secretless_server():
    x = X("n12_sparse")
    q, psi, S, L, N, d = x["q"], x["psi"], x["S"], x["L"], x["N"], x["d"]
    rot = {}
    for r in (1, S - 1):
        lead = x["cs"][0].multiKeySwitchGen(None, r)
        rot[r] = x["cs"][0].multiAddEvalKeys([lead, x["cs"][1].multiKeySwitchGen(lead, r)])
        ref = MK.protocol(x["seeds"], x["sks"], q, psi, indices=(r,))[1][r]
        assert np.array_equal(rot[r], ref)
    server = _server(x, _new_sparse, rot=rot)
    v = np.random.default_rng(12).uniform(-1, 1, S)
    ct = D.encrypt(server, torch.tensor(v, dtype=torch.float64, device="cuda"))
    assert ct.shape == (1, 2, L, N)
    for r in (1, S - 1):
        got = D.rotate(server, ct, r)
        ref = R.rotate_ref(_u64(ct), r, rot[r], q, psi)
        assert np.array_equal(_u64(got), ref), r
        parts = [D.partial_decrypt(c, got, i == 0) for i, c in enumerate(x["cs"])]
        dec = D.fuse_decrypt(server, parts, S, d).cpu().numpy()
        assert np.array_equal(dec, O.decrypt_vector(ref, x["sk_sum"], q, psi, S, d, S)), r
        err = np.abs(dec - np.roll(v, -r)).max()
        print("multikey sparse rotate %d: max error %.3g" % (r, err))
        assert err < 1e-6, r


# ------------------------------------------ C. key add: lanes, seams, positions, values ----
def _add_keys(x, n=3):
    """n valid uniform keys with equal a-vectors (fresh copies: the sweeps plant into them)."""
    keys = [_uniform(x, 10 + i) for i in range(n)]
    for k in keys[1:]:
        k[1] = keys[0][1]
    return keys


def _check_add_position(x, keys, which, pos, accept=True):
    """One position of the sweep: q_t there is refused by both calls; q_t - 1 is accepted by both and summed."""
    c, q, N = x["cs"][0], x["q"], x["N"]
    v, t = pos[0], pos[2]
    qt = int(x["mods"][t])
    with plant(keys[which], pos, qt):
        refused(lambda: c.multiAddEvalKeys(keys))
        refused(lambda: c.multiAddEvalMultKeys(keys))
    if not accept:
        return
    with plant(keys[which], pos, qt - 1):
        assert np.array_equal(c.multiAddEvalMultKeys(keys), MK.key_add(keys, q, N, sum_a=True)), (which, pos)
        with contextlib.ExitStack() as st:
            if v == 1:  # the a-vectors must stay equal there: the same word in every key
                for k in keys:
                    st.enter_context(plant(k, pos, qt - 1))
            assert np.array_equal(c.multiAddEvalKeys(keys), MK.key_add(keys, q, N)), (which, pos)


@pytest.mark.parametrize("j", [0, 1])
@pytest.mark.parametrize("v", [0, 1])
def test_key_add_position_sweep(v, j):
    """n11_L3: every tower and both lanes at both ends of a tower, in the first, a middle and the last key."""
    x = X("n11_L3")
    assert x["dn"] == 2
    keys = _add_keys(x)
    base = [k.copy() for k in keys]
    for pos in positions(x):
        if pos[:2] == (v, j):
            for which in range(3):
                _check_add_position(x, keys, which, pos)
    for k, b in zip(keys, base):
        assert np.array_equal(k, b)


@pytest.mark.parametrize("sid", ["n12_L12", "n12_L4_30bit"])
def test_key_add_lanes_on_the_other_chains(sid):
    """Every lane of the corners sweep, in the first key and in the last: q_t refused word by word; q_t - 1 at
    all of those words at once accepted and summed."""
    x = X(sid)
    c, q, N, mods = x["cs"][0], x["q"], x["N"], x["mods"]
    keys = _add_keys(x)
    sweep = corners(x)
    for which in (0, 2):
        for pos in sweep:
            _check_add_position(x, keys, which, pos, accept=False)
        with plant_all(keys[which], sweep, lambda t: int(mods[t]) - 1):
            assert np.array_equal(c.multiAddEvalMultKeys(keys), MK.key_add(keys, q, N, sum_a=True)), which
            with contextlib.ExitStack() as st:  # equal a-vectors: the same words in every key
                for k in keys:
                    st.enter_context(plant_all(k, [p for p in sweep if p[0] == 1], lambda t: int(mods[t]) - 1))
                assert np.array_equal(c.multiAddEvalKeys(keys), MK.key_add(keys, q, N)), which


def test_key_add_value_sweep():
    x = X("n11_L3")
    c = x["cs"][0]
    keys = _add_keys(x)
    seen_narrow = False
    for v in range(2):
        for t, w in value_places(x):
            for val in bad_values(x, t):
                seen_narrow |= val == int(x["mods"][0]) - 1
                for which in (0, 1, 2):
                    with plant(keys[which], (v, x["dn"] - 1, t, w), val):
                        refused(lambda: c.multiAddEvalKeys(keys))
                        refused(lambda: c.multiAddEvalMultKeys(keys))
    assert seen_narrow
    assert np.array_equal(c.multiAddEvalKeys(keys), MK.key_add(keys, x["q"], x["N"]))


@pytest.mark.parametrize("sid", ["n11_L3", "n12_L12", "n12_L4_30bit"])
def test_key_add_seam_between_b_and_a(sid):
    """The four words either side of half_words: the last pair of the b-vector (last digit, last tower of P)
    and the first pair of the a-vector (digit 0, tower 0)."""
    x = X(sid)
    c, q, N, mods = x["cs"][0], x["q"], x["N"], x["mods"]
    _, dn, T, _ = x["shape"]
    seam = [(0, dn - 1, T - 1, N - 2), (0, dn - 1, T - 1, N - 1), (1, 0, 0, 0), (1, 0, 0, 1)]
    keys = _add_keys(x)
    half = keys[0].size // 2
    flat = keys[1].reshape(-1)
    for i, pos in enumerate(seam):  # the flat words half - 2 .. half + 1
        with plant(keys[1], pos, 12345):
            assert flat[half - 2 + i] == 12345
    assert int(mods[T - 1]) != int(mods[0])  # a tower index carried across the seam compares with the wrong one
    for pos in seam:
        for which in range(3):
            _check_add_position(x, keys, which, pos)
        for val in bad_values(x, pos[2]):
            with plant(keys[1], pos, val):
                refused(lambda: c.multiAddEvalKeys(keys))
                refused(lambda: c.multiAddEvalMultKeys(keys))
    for pos in seam:
        t = pos[2]
        for which in (1, 2):
            other = (int(keys[which][pos]) + 1) % int(mods[t])  # differs, still canonical
            with plant(keys[which], pos, other):
                if pos[0] == 1:
                    refused(lambda: c.multiAddEvalKeys(keys), "a-vectors")
                else:
                    exp = MK.key_add(keys, q, N)
                    assert np.array_equal(c.multiAddEvalKeys(keys), exp)
                assert np.array_equal(c.multiAddEvalMultKeys(keys), MK.key_add(keys, q, N, sum_a=True))


def test_key_add_differing_a_sweep():
    """sum_a = False: one a-word that differs but is canonical, at every (digit, tower), in either lane, in a
    middle key and in the last one; with a bad residue planted as well, that message wins."""
    x = X("n11_L3")
    c, q, N, mods = x["cs"][0], x["q"], x["N"], x["mods"]
    _, dn, T, _ = x["shape"]
    keys = _add_keys(x)
    out = c.multiAddEvalKeys(keys)
    assert np.array_equal(out, MK.key_add(keys, q, N)) and np.array_equal(out[1], keys[0][1])
    for j in range(dn):
        for t in range(T):
            for w in (N // 2 + 2 * t, N // 2 + 2 * t + 1):
                for which in (1, 2):
                    pos = (1, j, t, w)
                    other = (int(keys[which][pos]) + 1) % int(mods[t])
                    with plant(keys[which], pos, other):
                        refused(lambda: c.multiAddEvalKeys(keys), "a-vectors")
                        assert np.array_equal(c.multiAddEvalMultKeys(keys), MK.key_add(keys, q, N, sum_a=True))
                        for bad in ((0, dn - 1 - j, t, w ^ 1), (1, j, (t + 1) % T, w)):
                            with plant(keys[3 - which], bad, int(mods[bad[2]])):
                                refused(lambda: c.multiAddEvalKeys(keys), "residue")
                                refused(lambda: c.multiAddEvalMultKeys(keys), "residue")
    # sum_a = False keeps the first key's a-vector even where later keys' b-vectors are anything
    assert np.array_equal(c.multiAddEvalKeys(keys)[1], keys[0][1])


SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


def _sentinel(x):
    out = np.arange(int(np.prod(x["shape"])), dtype=np.uint64).reshape(x["shape"])
    return out ^ SENTINEL


def test_refused_calls_leave_out_untouched_and_the_next_call_clean():
    """shelfi.h's contract through the C entry points: a refused call answers SHELFI_ERR_ARG and writes no
    word of `out`; the flag word is the call's own, so the next valid call on the same context -- of the same
    entry point or another -- answers 0 and the reference."""
    x = X("n11_L3")
    c, seed, sk, q, psi, N, mods = x["cs"][1], x["seeds"][1], x["sks"][1], x["q"], x["psi"], x["N"], x["mods"]
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(_lib.u64p)  # noqa: E731
    keys = _add_keys(x)
    arr = (_lib.u64p * 3)(*[p(k) for k in keys])
    prev, joint = _uniform(x, 20), _uniform(x, 21)
    T = x["shape"][2]
    good = {"add": lambda o: lib.shelfi_multi_add_eval_keys(c._ctx, arr, 3, 0, p(o)),
            "add_mult": lambda o: lib.shelfi_multi_add_eval_keys(c._ctx, arr, 3, 1, p(o)),
            "share": lambda o: lib.shelfi_multi_key_switch_gen(c._ctx, 1, p(prev), p(o)),
            "round2": lambda o: lib.shelfi_multi_mult_eval_key(c._ctx, p(joint), p(o))}
    ref = {"add": MK.key_add(keys, q, N), "add_mult": MK.key_add(keys, q, N, sum_a=True),
           "share": MK.share(seed, sk, q, psi, 1, prev), "round2": MK.round2(seed, joint, sk, q, psi)}
    # (the call, the array to plant in, where, what): a bad residue per entry point, and differing a-vectors
    faults = [("add", keys[1], (0, 1, 2, 7), int(mods[2])), ("add", keys[2], (1, 0, 0, 0), int(mods[0])),
              ("add", keys[2], (1, 1, T - 1, N - 1), int(keys[0][1, 1, T - 1, N - 1]) ^ 1),
              ("add_mult", keys[0], (1, 1, T - 1, N - 2), U64_MAX),
              ("share", prev, (0, 1, T - 1, 4), int(mods[T - 1])), ("share", prev, (1, 0, 0, N - 1), int(mods[0])),
              ("round2", joint, (0, 0, 1, 0), int(mods[1])), ("round2", joint, (1, 1, T - 1, N - 1), 1 << 63)]
    order = ["add", "share", "round2", "add_mult"]
    for i, (name, target, at, val) in enumerate(faults):
        out = _sentinel(x)
        with plant(target, at, val):
            assert good[name](out) == _lib.SHELFI_ERR_ARG, (name, at)
            assert np.array_equal(out, _sentinel(x)), (name, at)
            assert good[name](out) == _lib.SHELFI_ERR_ARG and np.array_equal(out, _sentinel(x))  # and again
        for nxt in (name, order[i % 4]):  # the very next valid call: the same entry point, then another
            assert good[nxt](out) == 0, (name, nxt)
            assert np.array_equal(out, ref[nxt]), (name, nxt)
            out = _sentinel(x)


# ------------------------------------------- D. round 2 and share imports, by position ----
@pytest.mark.parametrize("sid", ["n11_L3", "n12_L12", "n12_L4_30bit"])
def test_round2_position_sweep(sid):
    x = X(sid)
    c, seed, sk, q, psi = x["cs"][1], x["seeds"][1], x["sks"][1], x["q"], x["psi"]
    terms = MK.round2_terms(seed, sk, q, psi)
    joint = _uniform(x, 30)
    assert np.array_equal(c.multiMultEvalKey(joint), MK.round2(seed, joint, sk, q, psi))
    full_sweep = sid == "n11_L3"
    sweep = positions(x) if full_sweep else corners(x)
    for pos in sweep:
        qt = int(x["mods"][pos[2]])
        with plant(joint, pos, qt):
            refused(lambda: c.multiMultEvalKey(joint))
        if full_sweep:
            with plant(joint, pos, qt - 1):
                assert np.array_equal(c.multiMultEvalKey(joint), MK.round2_from_terms(terms, joint)), pos
    with plant_all(joint, sweep, lambda t: int(x["mods"][t]) - 1):  # q_t - 1 at every word of the sweep at once
        assert np.array_equal(c.multiMultEvalKey(joint), MK.round2(seed, joint, sk, q, psi))
    if sid == "n11_L3":
        for v, j in ((0, 0), (1, 1)):
            for t, w in value_places(x):
                for val in bad_values(x, t):
                    with plant(joint, (v, j, t, w), val):
                        refused(lambda: c.multiMultEvalKey(joint))
    assert np.array_equal(c.multiMultEvalKey(joint), MK.round2_from_terms(terms, joint))


@pytest.mark.parametrize("rk", ["0", "-(S-1)"])
@pytest.mark.parametrize("sid", ["n11_L3", "n12_L12", "n12_L4_30bit"])
def test_share_prev_position_sweep(sid, rk):
    """prev's a-vector and its b-vector, in every digit and tower (a bad b-word in digit 1 and in a tower of
    P among them)."""
    x = X(sid)
    c, seed, sk, q, psi = x["cs"][1], x["seeds"][1], x["sks"][1], x["q"], x["psi"]
    r = _index(x, rk) if rk != "0" else 0
    terms = MK.share_terms(seed, sk, q, psi, r)
    prev = _uniform(x, 31)
    base = c.multiKeySwitchGen(prev, r)
    assert np.array_equal(base, MK.share(seed, sk, q, psi, r, prev))
    full_sweep = sid == "n11_L3"
    sweep = positions(x) if full_sweep else corners(x)
    assert (0, 1, x["shape"][2] - 1, 1) in sweep
    for pos in sweep:
        qt = int(x["mods"][pos[2]])
        with plant(prev, pos, qt):
            refused(lambda: c.multiKeySwitchGen(prev, r))
        if full_sweep:
            with plant(prev, pos, qt - 1):
                got = c.multiKeySwitchGen(prev, r)
                assert np.array_equal(got, MK.share_from_terms(terms, prev)), pos
                assert pos[0] == 1 or np.array_equal(got, base)
    with plant_all(prev, sweep, lambda t: int(x["mods"][t]) - 1):  # q_t - 1 at every word of the sweep at once
        assert np.array_equal(c.multiKeySwitchGen(prev, r), MK.share(seed, sk, q, psi, r, prev))
    if sid == "n11_L3":
        for v, j in ((0, 1), (1, 0)):
            for t, w in value_places(x):
                for val in bad_values(x, t):
                    with plant(prev, (v, j, t, w), val):
                        refused(lambda: c.multiKeySwitchGen(prev, r))


@pytest.mark.parametrize("sid", G.SMALL)
def test_round2_of_planted_joint_keys(sid):
    x = X(sid)
    c, seed, sk, q, psi = x["cs"][0], x["seeds"][0], x["sks"][0], x["q"], x["psi"]
    En = MK.round2_terms(seed, sk, q, psi)[0]
    f, z = _full(x), np.zeros(x["shape"], np.uint64)
    last = x["dn"] - 1
    cases = {"b_full_a_zero": np.stack([f[0], z[1]]), "a_full_b_zero": np.stack([z[0], f[1]]), "one_digit": z.copy()}
    cases["one_digit"][:, last] = f[:, last]
    for name, joint in cases.items():
        out = c.multiMultEvalKey(joint)
        assert np.array_equal(out, MK.round2(seed, joint, sk, q, psi)), name
        zero = joint == 0
        assert zero.any() and np.array_equal(out[zero], En[zero]), name  # the zero half: its bare NTT(E)
        assert not (out[~zero] == En[~zero]).all(), name


# ------------------------------------ E. the protocol and the circuit where they had not run ----
WHOLE = [("n12_L12", 2), ("n12_L4_30bit", 3)]


def _tol(sid):
    sb = SHAPES[sid][2]
    return 1e-6 if sb == 52 else max(1e-7, 2.0 ** (18 - sb))


@pytest.mark.parametrize("sid,Pn", WHOLE, ids=str)
def test_protocol_keys_on_the_other_chains(sid, Pn):
    G.test_protocol_keys_equal_the_reference(sid, Pn)


@pytest.mark.parametrize("sid,Pn", WHOLE, ids=str)
def test_server_circuit_on_the_other_chains(sid, Pn):
    """test_server_circuit_under_joint_keys on the (3, 4, 4) chain and the 30-bit one, with the value tolerance
    of the scale (the module docstring has the oracle's own figures at 30 bits); the oracle's decrypt of the
    oracle's circuit is held to it first, so that a failure past that line is the device's."""
    x = X(sid, Pn)
    q, psi, N, S, L, d = x["q"], x["psi"], x["N"], x["S"], x["L"], x["d"]
    final, rot = G.joint_keys(sid, Pn)
    server = _server(x, lambda s: G._new(sid, s), final, rot)
    tol = _tol(sid)
    v = np.random.default_rng(Pn).uniform(-1, 1, S)
    ct = D.encrypt(server, torch.tensor(v, dtype=torch.float64, device="cuda"))
    ct_np = _u64(ct)
    ref_prod = O.eval_mult(ct_np, ct_np, final, q, psi)
    ref_sq = O.rescale(ref_prod, q, psi)
    refs = {"mult": (ref_sq, v * v), "rotate": (R.rotate_ref(ref_sq, 1, rot[1], q, psi), np.roll(v * v, -1)),
            "eval_sum": (R.eval_sum_ref(ref_sq, 4, rot, q, psi), sum(np.roll(v * v, -j) for j in range(4)))}
    scale = d * d / float(q[-1])
    ref_dec = {}
    for name, (ref, exp) in refs.items():
        ref_dec[name] = O.decrypt_vector(ref, x["sk_sum"][:L - 1], q[:L - 1], psi[:L - 1], S, scale, S)
        err = np.abs(ref_dec[name] - exp).max()
        print("multikey %s P=%d %s: the oracle's max error %.3g (tolerance %.3g)" % (sid, Pn, name, err, tol))
        assert err < tol, name
    prod = D.mult(server, ct, ct)
    assert np.array_equal(_u64(prod), ref_prod)
    sq = D.rescale(server, prod)
    assert np.array_equal(_u64(sq), ref_sq)
    outs = {"mult": sq, "rotate": D.rotate(server, sq, 1), "eval_sum": D.eval_sum(server, sq, 4)}
    for name, got in outs.items():
        assert np.array_equal(_u64(got), refs[name][0]), name
        parts = [D.partial_decrypt(c, got, i == 0) for i, c in enumerate(x["cs"])]
        assert parts[0].shape == (1, L - 1, N)
        dec = D.fuse_decrypt(server, parts, S, scale).cpu().numpy()
        assert np.array_equal(dec, ref_dec[name]), name
        assert np.abs(dec - refs[name][1]).max() < tol, name
    bound = x["dn"] * x["al"] * N * MK.mult_key_bound(N, Pn) + x["kP"] * (1 + N)
    defect = _relin_defect(_u64(prod), ct_np, ct_np, x["sk_sum"], q, psi)
    print("multikey %s P=%d: relinearization defect max |d| = %d (bound %d)" % (sid, Pn, defect, bound))
    assert defect <= bound


def test_protocol_and_mult_at_n15():
    """2^15 / L4, two parties: the EvalMult protocol and the joint rotation keys of 1 and S / 2 made share by
    share; mult and rescale on the server."""
    sid = "n15_L4"
    x = X(sid)
    cs, q, psi, S = x["cs"], x["q"], x["psi"], x["S"]
    shares = [cs[0].multiKeySwitchGen()]
    shares.append(cs[1].multiKeySwitchGen(shares[0]))
    mid = cs[0].multiAddEvalKeys(shares)
    final = cs[0].multiAddEvalMultKeys([c.multiMultEvalKey(mid) for c in cs])
    rot = {}
    for r in (1, S // 2):
        lead = cs[0].multiKeySwitchGen(None, r)
        rot[r] = cs[0].multiAddEvalKeys([lead, cs[1].multiKeySwitchGen(lead, r)])
    ref_final, ref_rot, ref_mid = MK.protocol(x["seeds"], x["sks"], q, psi, indices=(1, S // 2))
    assert np.array_equal(mid, ref_mid) and np.array_equal(final, ref_final)
    for r in rot:
        assert np.array_equal(rot[r], ref_rot[r]), r
    server = _server(x, lambda s: G._new(sid, s), final)
    v = np.random.default_rng(15).uniform(-1, 1, S)
    ct = D.encrypt(server, torch.tensor(v, dtype=torch.float64, device="cuda"))
    prod = D.mult(server, ct, ct)
    ref_prod = O.eval_mult(_u64(ct), _u64(ct), final, q, psi)
    assert np.array_equal(_u64(prod), ref_prod)
    assert np.array_equal(_u64(D.rescale(server, prod)), O.rescale(ref_prod, q, psi))


def test_mult_under_the_joint_key_below_the_top_level():
    """2^12 / L12 (alpha 4): the ciphertext walked down by squaring and rescaling under the joint key, as
    tests/test_gpu_f4_levels.py walks a single-key chain; at Ll = L - 1 (a partial last digit), alpha + 1 and
    alpha (the digit boundary) and 1 (one tower) the product equals the oracle's and the parties' partials of
    it fuse to the oracle's decrypt under sum s_i."""
    sid, Pn = "n12_L12", 2
    x = X(sid, Pn)
    q, psi, N, S, L, al = x["q"], x["psi"], x["N"], x["S"], x["L"], x["al"]
    final, _ = G.joint_keys(sid, Pn)
    server = _server(x, lambda s: G._new(sid, s), final)
    v = np.random.default_rng(21).uniform(-1, 1, S)
    ct = D.encrypt(server, torch.tensor(v, dtype=torch.float64, device="cuda"))
    scale = x["d"]
    checked = []
    for Ll in range(L, 0, -1):
        assert ct.shape == (1, 2, Ll, N)
        prod = D.mult(server, ct, ct)
        if Ll in (L - 1, al + 1, al, 1):
            ref = O.eval_mult(_u64(ct), _u64(ct), final, q, psi)
            assert np.array_equal(_u64(prod), ref), Ll
            parts = [D.partial_decrypt(c, prod, i == 0) for i, c in enumerate(x["cs"])]
            assert parts[0].shape == (1, Ll, N)
            dec = D.fuse_decrypt(server, parts, S, scale * scale).cpu().numpy()
            exp = O.decrypt_vector(ref, x["sk_sum"][:Ll], q[:Ll], psi[:Ll], S, scale * scale, S)
            assert np.array_equal(dec, exp), Ll
            if Ll > 1:  # (at one tower the product, at scale ~2^104 under a 60-bit modulus, holds no value)
                v2 = v * v
                print("multikey walk Ll=%d: max error %.3g" % (Ll, np.abs(dec - v2).max()))
                assert np.abs(dec - v2).max() < 1e-6, Ll
            checked.append(Ll)
        if Ll > 1:
            ct = D.rescale(server, prod)
            scale = scale * scale / float(q[Ll - 1])
            v = v * v
    assert checked == [L - 1, al + 1, al, 1]


# ------------------------------------------ F. the key chain over planted previous keys ----
CHAIN_SHAPES = ("n11_L3", "n13_L3", "n12_L4_30bit")


def _pk_planted(x):
    q, N, L = x["q"], x["N"], x["L"]
    rng = np.random.default_rng([40, N])
    full = np.broadcast_to((q - np.uint64(1))[None, :, None], (2, L, N)).copy()
    uni = np.stack([rng.integers(0, int(qt), size=(2, N), dtype=np.uint64) for qt in q], axis=1)
    zero = np.zeros((2, L, N), np.uint64)
    return {"full": full, "zero": zero, "uniform": uni, "b_full_a_zero": np.stack([full[0], zero[1]])}


@pytest.mark.parametrize("sid", CHAIN_SHAPES)
def test_key_chain_over_planted_prev(sid):
    x = X(sid)
    q, psi = x["q"], x["psi"]
    seed = 4500 + x["N"]
    c = G._new(sid, seed)
    sks = []
    for name, prev in _pk_planted(x).items():
        c.multipartyKeyGen(prev)
        pk, sk = c.get_keys()
        ref_pk, ref_sk = MK.chain_step(seed, prev, q, psi)
        assert np.array_equal(pk[1], ref_pk[1]) and np.array_equal(pk[1], prev[1]), name
        assert np.array_equal(pk[0], ref_pk[0]), name
        assert np.array_equal(sk, ref_sk), name
        sks.append(sk)
    for sk in sks[1:]:
        assert np.array_equal(sk, sks[0])
    assert sks[0].any()


@pytest.mark.parametrize("sid", CHAIN_SHAPES)
def test_key_chain_refusal_sweep(sid):
    """The host range check of shelfi_multiparty_keygen: either vector, every tower, the first and the last
    word, q_t, q_t + 1, 2^64 - 1 and (in a tower narrower than tower 0) q_0 - 1 are refused with
    SHELFI_ERR_FORMAT and change nothing; q_t - 1 is accepted."""
    x = X(sid)
    q, psi, N, L = x["q"], x["psi"], x["N"], x["L"]
    seed = 4600 + N
    bare, keyed = G._new(sid, seed), G._new(sid, seed + 1)
    keyed.set_keys(x["pk"], x["sks"][0])
    held = [a.tobytes() for a in keyed.get_keys()]
    prev = _pk_planted(x)["uniform"]
    narrow = 0
    for v in range(2):
        for t in range(L):
            qt = int(q[t])
            vals = [qt, qt + 1, U64_MAX] + ([int(q[0]) - 1] if int(q[0]) - 1 >= qt else [])
            narrow += len(vals) == 4
            for w in (0, N - 1):
                for val in vals:
                    with plant(prev, (v, t, w), val):
                        for c in (bare, keyed):
                            with pytest.raises(m.ShelfiError) as ei:
                                c.multipartyKeyGen(prev)
                            assert ei.value.code == _lib.SHELFI_ERR_FORMAT, (v, t, w, val)
                assert not bare.info()["keys_loaded"]
                assert [a.tobytes() for a in keyed.get_keys()] == held
    assert narrow == 2 * (L - 1)  # every tower after the first is narrower in these chains
    for v in range(2):
        for t in range(L):
            for w in (0, N - 1):
                with plant(prev, (v, t, w), int(q[t]) - 1):
                    keyed.multipartyKeyGen(prev)
                    pk, sk = keyed.get_keys()
                    ref_pk, ref_sk = MK.chain_step(seed + 1, prev, q, psi)
                    assert np.array_equal(pk, ref_pk) and np.array_equal(sk, ref_sk), (v, t, w)
    assert not bare.info()["keys_loaded"]
