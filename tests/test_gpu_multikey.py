"""The multiparty EvalMult / rotation / EvalSum key protocols of threshold CKKS on the MI355X (DESIGN.md
§2.12; the reference's code/mkhe/mkhe.cpp:271-317): every key bit-exact against tests/multikey_ref.py
(held to its meaning by tests/test_multikey_ref.py) under the same seeds, the errors the keys hide
extracted exactly, and the joint keys installed on a server that holds no secret, where mult, rescale,
rotate and eval_sum equal the oracle's under the same keys and the parties' partial decryptions fuse to
the oracle's decrypt under sum s_i.

Shapes: 2^11 / L3 (one NTT block), 2^13 / L3 (a columns pass, a one-tower last digit), 2^12 / L4 at 30 /
45 bits (q < 2^40: the generic passes), 2^12 / L12 (T = 16, alpha 4, kP 4), 2^15 / L4, and 2^17 / L2 with
index -2, whose Galois element is above 2^16 (the 32-bit product g e wraps).

Bounds: a share's error is one CDT sample per coefficient, |e| < 64; the final EvalMult key's error
e s + E1 s + E2 is below B Pn (2 N Pn + 1) (multikey_ref.mult_key_bound); the relinearization defect
below dnum alpha N bound + kP (1 + N) (f4_cases.py's rule with that key bound); decoded values within
1e-6, tests/test_oracle_f4.py's tolerance for the same circuit at a 52-bit scale."""
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

# id: (ring, towers, scale bits, first modulus bits, (dnum, alpha, kP))
SHAPES = {
    "n11_L3": (1 << 11, 3, 52, 60, (2, 2, 2)),
    "n13_L3": (1 << 13, 3, 52, 60, (2, 2, 2)),
    "n12_L4_30bit": (1 << 12, 4, 30, 45, (2, 2, 2)),
    "n12_L12": (1 << 12, 12, 52, 60, (3, 4, 4)),
    "n15_L4": (1 << 15, 4, 52, 60, (2, 2, 2)),
    "n17_L2": (1 << 17, 2, 52, 60, (2, 1, 1)),
}
SMALL = ("n11_L3", "n12_L4_30bit", "n12_L12")
SHARE_CASES = [(sid, r) for sid in SHAPES for r in (0, 1, -2) if sid != "n17_L2" or r == -2]


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _new(sid, seed):
    N, L, sb, fb = SHAPES[sid][:4]
    return m.CKKS("ckks", N // 2, sb, "", multDepth=L - 1, firstModBits=fb, ringDim=N, seed=seed, decodeNoise=False)


@functools.lru_cache(maxsize=None)
def parties(sid, Pn):
    """Pn contexts of one shape, every one seeded differently, after the threshold key chain: party 0
    generates keys, the others chain multipartyKeyGen, all install (pk_joint, own share)."""
    seeds = [3100 + 10 * list(SHAPES).index(sid) + i for i in range(Pn)]
    cs = [_new(sid, s) for s in seeds]
    assert cs[0].genCryptoContextAndKeyGen() == 1
    keys = [cs[0].get_keys()]
    for c in cs[1:]:
        c.multipartyKeyGen(keys[-1][0])
        keys.append(c.get_keys())
    pk = keys[-1][0]
    for c, (_, sk) in zip(cs, keys):
        c.set_keys(pk, sk)
        c.set_threshold_noise(0.0)
    inf = cs[0].info()
    N, L = SHAPES[sid][:2]
    assert (inf["ring_dim"], inf["num_towers"]) == (N, L)
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    dn, al, p, _ = O.special_primes(N, q)
    assert (dn, al, len(p)) == SHAPES[sid][4]
    mods = np.array([int(v) for v in q] + [int(v) for v in p], np.uint64)
    sks = [k[1] for k in keys]
    return dict(cs=cs, seeds=seeds, sks=sks, pk=pk, q=q, psi=psi, N=N, L=L, S=inf["batch"], d=inf["delta"],
                dn=dn, al=al, kP=len(p), mods=mods, sk_sum=MK.sk_sum(sks, q), shape=(2, dn, L + len(p), N))


def _uniform_key(rng, x):
    out = np.empty(x["shape"], np.uint64)
    for t, mt in enumerate(x["mods"]):
        out[:, :, t] = rng.integers(0, int(mt), size=(2, x["dn"], x["N"]), dtype=np.uint64)
    return out


def _full_key(x):
    out = np.empty(x["shape"], np.uint64)
    out[:] = (x["mods"] - np.uint64(1))[None, None, :, None]
    return out


# --------------------------------------------------------------------- shares ----
@pytest.mark.parametrize("sid,r", SHARE_CASES, ids=str)
def test_share_bitexact_lead_and_follower(sid, r):
    x = parties(sid, 2)
    (c0, c1), (s0, s1), (sk0, sk1) = x["cs"], x["seeds"], x["sks"]
    q, psi = x["q"], x["psi"]
    lead = c0.multiKeySwitchGen(None, r)
    assert lead.shape == x["shape"] and lead.dtype == np.uint64
    assert np.array_equal(lead, MK.share(s0, sk0, q, psi, r))
    foll = c1.multiKeySwitchGen(lead, r)
    assert np.array_equal(foll[1], lead[1])  # the a-vector, bit for bit
    assert np.array_equal(foll, MK.share(s1, sk1, q, psi, r, lead))
    for key, sk in ((lead, sk0), (foll, sk1)):
        e = MK.switch_key_error(key, r, sk, q, psi)
        assert (e == e[:, :1]).all()
        assert np.abs(e).max() < MK.B_ERR and all(e[j].any() for j in range(x["dn"]))
    assert np.array_equal(c0.multiKeySwitchGen(index=r), lead)  # the same seed: the same share


def test_share_streams_are_their_own():
    """Under one seed a share reuses no (a, e) of the single-key rotation key (domain 6) or of the
    EvalMult key (domain 4); the EvalMult share (g = 1) and a rotation share differ; unseeded, two
    calls differ."""
    x = parties("n11_L3", 2)
    c, sk, q, psi = x["cs"][0], x["sks"][0], x["q"], x["psi"]
    twin = _new("n11_L3", x["seeds"][0])
    twin.set_keys(x["pk"], sk)
    twin.rotationKeyGen([1])
    twin.evalMultKeyGen()
    rot, evk = twin.get_rotation_key(1), twin.get_eval_key()
    sh1, sh0 = c.multiKeySwitchGen(None, 1), c.multiKeySwitchGen(None, 0)
    e_sh1, e_sh0 = MK.switch_key_error(sh1, 1, sk, q, psi), MK.switch_key_error(sh0, 0, sk, q, psi)
    e_rot, e_evk = R.key_error(rot, 1, sk, q, psi), MK.switch_key_error(evk, "mult", sk, q, psi)
    for a, b in ((e_sh1, e_rot), (e_sh1, e_evk), (e_sh0, e_rot), (e_sh0, e_evk), (e_sh0, e_sh1)):
        assert not (a[:, 0] == b[:, 0]).all(axis=-1).any()
    for a, b in ((sh1, rot), (sh1, evk), (sh0, rot), (sh0, evk), (sh0, sh1)):
        assert not (a[1] == b[1]).all(axis=-1).any()
    loose = _new("n11_L3", 0)
    loose.set_keys(x["pk"], sk)
    k1, k2 = loose.multiKeySwitchGen(), loose.multiKeySwitchGen()
    assert not (k1 == k2).all(axis=-1).any()
    f1, f2 = loose.multiKeySwitchGen(k1), loose.multiKeySwitchGen(k1)
    assert np.array_equal(f1[1], f2[1]) and not (f1[0] == f2[0]).all(axis=-1).any()
    r1, r2 = loose.multiMultEvalKey(k1), loose.multiMultEvalKey(k1)
    assert not (r1 == r2).all(axis=-1).any()


# ------------------------------------------------------------------------ add ----
@pytest.mark.parametrize("n", [1, 2, 3, 16])
@pytest.mark.parametrize("sid", SMALL)
def test_key_add(sid, n):
    x = parties(sid, 2)
    c, N, q = x["cs"][0], x["N"], x["q"]
    rng = np.random.default_rng([n, N])
    keys = [_uniform_key(rng, x) for _ in range(n)]
    assert np.array_equal(c.multiAddEvalMultKeys(keys), MK.key_add(keys, q, N, sum_a=True))
    for k in keys[1:]:
        k[1] = keys[0][1]
    assert np.array_equal(c.multiAddEvalKeys(keys), MK.key_add(keys, q, N))
    full = [_full_key(x) for _ in range(n)]  # the largest sums: n (q_t - 1) in every word
    exp = MK.key_add(full, q, N, sum_a=True)
    assert np.array_equal(exp[0, 0, :, 0], x["mods"] - np.uint64(n))  # n (q_t - 1) = -n mod q_t
    assert np.array_equal(c.multiAddEvalMultKeys(full), exp)
    assert np.array_equal(c.multiAddEvalKeys(full), MK.key_add(full, q, N))
    if n > 1:  # one word of the last tower's a differs, in the last key
        keys[-1] = keys[-1].copy()
        keys[-1][1, -1, -1, -1] ^= np.uint64(1)
        if keys[-1][1, -1, -1, -1] >= x["mods"][-1]:
            keys[-1][1, -1, -1, -1] -= np.uint64(2)
        with pytest.raises(ValueError, match="a-vectors"):
            c.multiAddEvalKeys(keys)
        c.multiAddEvalMultKeys(keys)  # summed there: no comparison
    for v, t in ((0, 0), (1, x["shape"][2] - 1)):  # a word equal to its modulus, in either vector
        bad = [k.copy() for k in full]
        bad[-1][v, -1, t, 5] = x["mods"][t]
        for call in (c.multiAddEvalKeys, c.multiAddEvalMultKeys):
            with pytest.raises(ValueError, match="residue"):
                call(bad)


def test_key_add_refuses_seventeen_keys():
    x = parties("n11_L3", 2)
    c = x["cs"][0]
    key = _full_key(x)
    with pytest.raises(ValueError, match="16"):
        c.multiAddEvalKeys([key] * 17)
    lib = _lib.load()
    arr = (_lib.u64p * 17)(*[key.ctypes.data_as(_lib.u64p)] * 17)
    out = np.zeros_like(key)
    for n in (17, 0):
        assert lib.shelfi_multi_add_eval_keys(c._ctx, arr, n, 0, out.ctypes.data_as(_lib.u64p)) == _lib.SHELFI_ERR_ARG
    assert not out.any()
    assert lib.shelfi_multi_add_eval_keys(c._ctx, arr, 16, 0, out.ctypes.data_as(_lib.u64p)) == 0


# -------------------------------------------------------------------- round 2 ----
@pytest.mark.parametrize("sid", list(SHAPES))
def test_round2_bitexact(sid):
    x = parties(sid, 2)
    c, seed, sk, q, psi = x["cs"][1], x["seeds"][1], x["sks"][1], x["q"], x["psi"]
    joint = _uniform_key(np.random.default_rng(x["N"]), x)
    assert np.array_equal(c.multiMultEvalKey(joint), MK.round2(seed, joint, sk, q, psi))
    if sid in SMALL:
        full = _full_key(x)
        assert np.array_equal(c.multiMultEvalKey(full), MK.round2(seed, full, sk, q, psi))
    bad = joint.copy()
    bad[1, -1, -1, -1] = x["mods"][-1]
    with pytest.raises(ValueError, match="residue"):
        c.multiMultEvalKey(bad)


@pytest.mark.parametrize("sid", SMALL)
def test_round2_of_a_zero_key_is_its_errors(sid):
    """A zero joint key leaves NTT(E2), NTT(E1): one small polynomial per digit and vector, the same in
    every tower, all distinct."""
    x = parties(sid, 2)
    c, seed = x["cs"][0], x["seeds"][0]
    out = c.multiMultEvalKey(np.zeros(x["shape"], np.uint64))
    _, mods, roots = R.s_ext(x["sks"][0], x["q"], x["psi"])
    E = np.empty(x["shape"], np.int64)
    for idx in np.ndindex(*x["shape"][:3]):
        E[idx] = O.to_signed(O.ntt_inv(out[idx], mods[idx[2]], roots[idx[2]]), mods[idx[2]])
    assert (E == E[:, :, :1]).all()
    assert np.array_equal(E[:, :, 0], MK.round2_errors(seed, x["N"], x["dn"]))
    flat = E[:, :, 0].reshape(-1, x["N"])
    assert np.abs(flat).max() < MK.B_ERR and flat.any(axis=1).all()
    assert len({row.tobytes() for row in flat}) == len(flat)


# ------------------------------------------------------------- whole protocol ----
PROTOCOLS = [("n11_L3", 3), ("n13_L3", 3), ("n11_L3", 16), ("n11_L3", 1)]


@functools.lru_cache(maxsize=None)
def joint_keys(sid, Pn):
    """The protocol on the device: -> (final EvalMult key, {index: joint EvalSum key})."""
    x = parties(sid, Pn)
    shares, maps = [], []
    for c in x["cs"]:
        shares.append(c.multiKeySwitchGen(shares[-1] if shares else None))
        maps.append(c.multiEvalSumKeyGen(maps[-1] if maps else None))
    lead = x["cs"][0]
    mid = lead.multiAddEvalKeys(shares)
    final = lead.multiAddEvalMultKeys([c.multiMultEvalKey(mid) for c in x["cs"]])
    return final, lead.multiAddEvalSumKeys(maps)


@pytest.mark.parametrize("sid,Pn", PROTOCOLS, ids=str)
def test_protocol_keys_equal_the_reference(sid, Pn):
    x = parties(sid, Pn)
    q, psi, N, S = x["q"], x["psi"], x["N"], x["S"]
    final, rot = joint_keys(sid, Pn)
    assert sorted(rot) == [1 << i for i in range(S.bit_length() - 1)]
    ref_final, ref_rot, _ = MK.protocol(x["seeds"], x["sks"], q, psi, indices=sorted(rot))
    assert np.array_equal(final, ref_final)
    for r in rot:
        assert np.array_equal(rot[r], ref_rot[r]), r
    err = MK.switch_key_error(final, "mult", x["sk_sum"], q, psi)
    assert (err == err[:, :1]).all()
    worst = int(np.abs(err).max())
    print("multikey %s P=%d: final EvalMult key max |err| = %d (bound %d)" % (sid, Pn, worst,
                                                                            MK.mult_key_bound(N, Pn)))
    assert 0 < worst < MK.mult_key_bound(N, Pn)
    for r in (1, S // 2):
        e = R.key_error(rot[r], r, x["sk_sum"], q, psi)
        assert (e == e[:, :1]).all() and 0 < np.abs(e).max() < MK.B_ERR * Pn


@pytest.mark.parametrize("sid,Pn", PROTOCOLS, ids=str)
def test_server_circuit_under_joint_keys(sid, Pn):
    """A server with the joint public key and no secret: mult, rescale, rotate, eval_sum equal the oracle's
    under the same keys; sigma = 0 partials of every party at L - 1 towers fuse to the oracle's decrypt
    under sum sk_i; the relinearization identity holds on the device's output."""
    x = parties(sid, Pn)
    q, psi, N, S, L, d = x["q"], x["psi"], x["N"], x["S"], x["L"], x["d"]
    final, rot = joint_keys(sid, Pn)
    server = _new(sid, 4242)
    server.set_keys(x["pk"], np.zeros((L, N), np.uint64))
    server.set_eval_key(final)
    for r, key in rot.items():
        server.set_rotation_key(r, key)
    v = np.random.default_rng(Pn).uniform(-1, 1, S)
    ct = D.encrypt(server, torch.tensor(v, dtype=torch.float64, device="cuda"))
    ct_np = _u64(ct)
    prod = D.mult(server, ct, ct)
    ref_prod = O.eval_mult(ct_np, ct_np, final, q, psi)
    assert np.array_equal(_u64(prod), ref_prod)
    sq = D.rescale(server, prod)
    ref_sq = O.rescale(ref_prod, q, psi)
    assert np.array_equal(_u64(sq), ref_sq)
    outs = {"mult": (sq, ref_sq, v * v),
            "rotate": (D.rotate(server, sq, 1), R.rotate_ref(ref_sq, 1, rot[1], q, psi), np.roll(v * v, -1)),
            "eval_sum": (D.eval_sum(server, sq, 4), R.eval_sum_ref(ref_sq, 4, rot, q, psi),
                         sum(np.roll(v * v, -j) for j in range(4)))}
    scale = d * d / float(q[-1])
    for name, (got, ref, exp) in outs.items():
        assert np.array_equal(_u64(got), ref), name
        parts = [D.partial_decrypt(c, got, i == 0) for i, c in enumerate(x["cs"])]
        assert parts[0].shape == (1, L - 1, N)
        dec = D.fuse_decrypt(server, parts, S, scale).cpu().numpy()
        assert np.array_equal(dec, O.decrypt_vector(ref, x["sk_sum"][:L - 1], q[:L - 1], psi[:L - 1], S, scale, S))
        err = np.abs(dec - exp).max()
        print("multikey %s P=%d %s: max error %.3g" % (sid, Pn, name, err))
        assert err < 1e-6, name
    bound = x["dn"] * x["al"] * N * MK.mult_key_bound(N, Pn) + x["kP"] * (1 + N)
    defect = _relin_defect(_u64(prod), ct_np, ct_np, x["sk_sum"], q, psi)
    print("multikey %s P=%d: relinearization defect max |d| = %d (bound %d)" % (sid, Pn, defect, bound))
    assert defect <= bound


# --------------------------------------------------------------------- guards ----
def test_guards():
    x = parties("n11_L3", 2)
    c, shape = x["cs"][0], x["shape"]
    key = c.multiKeySwitchGen()
    # no key pair
    bare = _new("n11_L3", 5)
    with pytest.raises(RuntimeError):
        bare.multiKeySwitchGen()
    with pytest.raises(RuntimeError):
        bare.multiMultEvalKey(key)
    assert np.array_equal(bare.multiAddEvalKeys([key]), key)  # the server's step: no keys needed
    # indices
    for r in (x["S"], -x["S"]):
        with pytest.raises(ValueError, match="batch"):
            c.multiKeySwitchGen(None, r)
    # shapes and dtypes
    wrong = [key[:1], key.reshape(-1), key.astype(np.int64), key.astype(np.float64), key[..., :-1],
             np.zeros(shape[:2] + (shape[2] + 1, shape[3]), np.uint64)]
    for w in wrong:
        for call in (lambda: c.multiKeySwitchGen(w), lambda: c.multiMultEvalKey(w), lambda: c.multiAddEvalKeys([w]),
                     lambda: c.multiAddEvalKeys([key, w]), lambda: c.multiAddEvalMultKeys([key, w])):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        c.multiAddEvalKeys([])
    with pytest.raises(ValueError):
        c.multiEvalSumKeyGen({1: key})
    with pytest.raises(ValueError):
        c.multiAddEvalSumKeys([{1: key}, {2: key}])
    # an imported previous key with a word equal to its modulus, in either vector
    for v, t in ((0, 0), (1, shape[2] - 1)):
        bad = key.copy()
        bad[v, 0, t, 3] = x["mods"][t]
        with pytest.raises(ValueError, match="residue"):
            c.multiKeySwitchGen(bad)
    # NULL out
    lib = _lib.load()
    p = key.ctypes.data_as(_lib.u64p)
    assert lib.shelfi_multi_key_switch_gen(c._ctx, 0, None, None) == _lib.SHELFI_ERR_ARG
    assert lib.shelfi_multi_mult_eval_key(c._ctx, p, None) == _lib.SHELFI_ERR_ARG
    assert lib.shelfi_multi_mult_eval_key(c._ctx, None, p) == _lib.SHELFI_ERR_ARG
    arr = (_lib.u64p * 1)(p)
    assert lib.shelfi_multi_add_eval_keys(c._ctx, arr, 1, 0, None) == _lib.SHELFI_ERR_ARG
    assert lib.shelfi_multi_add_eval_keys(c._ctx, None, 1, 0, p) == _lib.SHELFI_ERR_ARG
    # nothing is installed by any of it
    assert c.rotation_key_indices() == [] and not c.eval_key_info()["has_key"]


def test_chain_too_long_is_refused_by_name():
    """tests/f4_cases.py's 13-tower chain: 5 special primes, 18 towers."""
    c = m.CKKS("ckks", 2048, 52, "", multDepth=12, firstModBits=60, ringDim=4096, seed=1213, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    dn, al, p, _ = O.special_primes(4096, np.array(c.info()["moduli"], np.uint64))
    assert (dn, al, len(p)) == (3, 5, 5)
    key = np.zeros((2, dn, 13 + len(p), 4096), np.uint64)
    for call in (lambda: c.multiKeySwitchGen(), lambda: c.multiKeySwitchGen(key, 1), lambda: c.multiEvalSumKeyGen(),
                 lambda: c.multiMultEvalKey(key), lambda: c.multiAddEvalKeys([key]),
                 lambda: c.multiAddEvalMultKeys([key, key])):
        with pytest.raises(ValueError, match="<= 16"):
            call()
        assert c.rotation_key_indices() == [] and not c.eval_key_info()["has_key"]


def test_existing_keygen_is_unchanged_by_share_calls():
    """evalMultKeyGen / rotationKeyGen under a seed give the same bytes before and after share calls on the
    same context, and the oracle's EvalMult key."""
    x = parties("n13_L3", 2)
    c = _new("n13_L3", 77)
    c.set_keys(x["pk"], x["sks"][0])
    c.evalMultKeyGen()
    c.rotationKeyGen([1, -2])
    before = (c.get_eval_key(), c.get_rotation_key(1), c.get_rotation_key(-2))
    assert np.array_equal(before[0], O.evk_keygen(77, x["sks"][0], x["q"], x["psi"]))
    sh = c.multiKeySwitchGen()
    c.multiKeySwitchGen(sh, 1)
    c.multiMultEvalKey(sh)
    held = (c.get_eval_key(), c.get_rotation_key(1), c.get_rotation_key(-2))
    c.evalMultKeyGen()
    c.rotationKeyGen([1, -2])
    after = (c.get_eval_key(), c.get_rotation_key(1), c.get_rotation_key(-2))
    for a, b, k in zip(before, held, after):
        assert np.array_equal(a, b) and np.array_equal(a, k)
