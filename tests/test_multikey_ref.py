"""tests/multikey_ref.py held to its meaning on the CPU: its restated sampler
reproduces the oracle's EvalMult key draw; the keys its protocol makes hide one small integer
polynomial per digit, the same in every tower of Q u P and below the worst-case bound; and the
oracle's EvalMult / ModReduce and the rotation reference under those keys decode under sum s_i to
x^2, its roll and its windowed sum.  The helpers of tests/test_gpu_multikey_edges.py (planted keys, the
share and round-2 references with their NTTs done once, chain_step, the first index whose Galois element
passes a bound) are held to the same parts, and a sparse batch rotates under joint keys.  And, with no
device: the library exports the three entry points and they refuse a NULL context."""
import ctypes as C
import functools

import numpy as np
import pytest

import multikey_ref as MK
import oracle as O
import rotation_ref as R

# (ring, towers, scale bits, first modulus bits, parties)
CASES = [(2048, 3, 52, 60, 1), (2048, 3, 52, 60, 3), (2048, 3, 52, 60, 16), (4096, 4, 30, 45, 3)]
IDS = ["n11_L3_P1", "n11_L3_P3", "n11_L3_P16", "n12_L4_30bit_P3"]


def test_stream_words_are_chacha20_blocks():
    key = O.seed_to_key(77)
    nonce = (7 << 56) | (5 << 24) | (1 << 16) | 3
    w = MK.stream_words(key, nonce, 40)
    for blk in range(5):
        b = O.chacha20_block(key, blk, nonce).astype(np.uint64)
        assert np.array_equal(w[8 * blk:8 * blk + 8], b[0::2] | (b[1::2] << np.uint64(32)))


@pytest.mark.parametrize("N,L,sb,fb", [(2048, 3, 52, 60), (4096, 4, 30, 45)])
def test_sampler_reproduces_the_oracle_evaluation_key(N, L, sb, fb):
    """At nonce base 4 << 56 the restated draw is or_evk_keygen's: the same a, and the errors its key
    hides (b + a s - [digit] P s^2, as R.key_error extracts a rotation key's)."""
    q, psi = O.params_generate(N, L, sb, fb)
    s, e, a = O.sample_keygen(3, N, q)
    sk, _ = O.keygen(s, e, a, q, psi)
    evk = O.evk_keygen(21, sk, q, psi)
    _, mods, _ = R.s_ext(sk, q, psi)
    err = MK.switch_key_error(evk, "mult", sk, q, psi)
    key = O.seed_to_key(21)
    for j in range(evk.shape[1]):
        ej, aj = MK.sample_digit(key, 4 << 56, j, N, mods)
        assert np.array_equal(aj, evk[1, j])
        assert (err[j] == ej[None]).all()
        assert 0 < np.abs(ej).max() < MK.B_ERR


@functools.lru_cache(maxsize=None)
def _setup(cid):
    N, L, sb, fb, Pn = CASES[IDS.index(cid)]
    q, psi = O.params_generate(N, L, sb, fb)
    seeds = [100 + 7 * i for i in range(Pn)]
    ss, sks = [], []
    for sd in seeds:
        s, e, a = O.sample_keygen(sd, N, q)
        ss.append(s)
        sks.append(O.keygen(s, e, a, q, psi)[0])
    # the joint key pair of sum s_i (any e, a: the chain's are pinned by test_gpu_threshold.py)
    _, e, a = O.sample_keygen(999, N, q)
    sk_joint, pk = O.keygen(sum(ss), e, a, q, psi)
    assert np.array_equal(sk_joint, MK.sk_sum(sks, q))
    final, rot, mid = MK.protocol(seeds, sks, q, psi, indices=(1, 2))
    return dict(N=N, L=L, sb=sb, Pn=Pn, q=q, psi=psi, seeds=seeds, sks=sks, sk=sk_joint, pk=pk, final=final,
                rot=rot, mid=mid)


@pytest.mark.parametrize("cid", IDS)
def test_joint_keys_hide_one_small_error(cid):
    x = _setup(cid)
    N, Pn, q, psi, sk = x["N"], x["Pn"], x["q"], x["psi"], x["sk"]
    err = MK.switch_key_error(x["final"], "mult", sk, q, psi)
    assert (err == err[:, :1]).all()
    worst = int(np.abs(err).max())
    print("final EvalMult key %s: max |err| = %d (bound %d)" % (cid, worst, MK.mult_key_bound(N, Pn)))
    assert 0 < worst < MK.mult_key_bound(N, Pn)
    # round 1's sum: a key from s to s with the parties' errors summed
    e1 = MK.switch_key_error(x["mid"], 0, sk, q, psi)
    assert (e1 == e1[:, :1]).all() and 0 < np.abs(e1).max() < MK.B_ERR * Pn
    for r, key in x["rot"].items():
        er = MK.switch_key_error(key, r, sk, q, psi)
        assert (er == er[:, :1]).all() and 0 < np.abs(er).max() < MK.B_ERR * Pn, r
        assert np.array_equal(key[1], MK.share(x["seeds"][0], x["sks"][0], q, psi, r)[1])  # the lead's a
    # no (a, e) pair shared with the single-key EvalMult key (domain 4) of the lead's seed
    evk = O.evk_keygen(x["seeds"][0], x["sks"][0], q, psi)
    assert not (x["mid"][1] == evk[1]).all(axis=-1).any()


@pytest.mark.parametrize("cid", IDS[:3])
def test_circuit_under_joint_keys_decodes_under_the_joint_secret(cid):
    """mult -> rescale -> rotate / eval_sum(4) under the protocol's keys, decrypted with sum sk_i; the
    tolerance is tests/test_oracle_f4.py's for the same circuit (52-bit scale)."""
    x = _setup(cid)
    N, L, q, psi, sk = x["N"], x["L"], x["q"], x["psi"], x["sk"]
    S, d = N // 2, float(q[-1])
    v = np.random.default_rng(5).uniform(-1, 1, S)
    ct = O.encrypt_vector(v, x["pk"], q, psi, N, S, d, seed=8)
    sq = O.rescale(O.eval_mult(ct, ct, x["final"], q, psi), q, psi)
    scale = d * d / float(q[-1])

    def dec(c):
        return O.decrypt_vector(c, sk[:L - 1], q[:L - 1], psi[:L - 1], S, scale, S)

    errs = [np.abs(dec(sq) - v * v).max(),
            np.abs(dec(R.rotate_ref(sq, 1, x["rot"][1], q, psi)) - np.roll(v * v, -1)).max(),
            np.abs(dec(R.eval_sum_ref(sq, 4, x["rot"], q, psi)) - sum(np.roll(v * v, -j) for j in range(4))).max()]
    print("%s: max error mult %.3g, rotate %.3g, eval_sum(4) %.3g" % ((cid,) + tuple(errs)))
    assert max(errs) < 1e-6


def test_library_exports_the_multiparty_key_calls():
    """No device: the three entry points exist and answer SHELFI_ERR_ARG for a NULL context."""
    from SHELFI_FHE import _lib

    lib = _lib.load()
    for name in ("shelfi_multi_key_switch_gen", "shelfi_multi_add_eval_keys", "shelfi_multi_mult_eval_key"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    buf = np.zeros(4, np.uint64)
    p = buf.ctypes.data_as(_lib.u64p)
    arr = (_lib.u64p * 1)(p)
    assert lib.shelfi_multi_key_switch_gen(None, 0, None, p) == _lib.SHELFI_ERR_ARG
    assert lib.shelfi_multi_add_eval_keys(None, arr, 1, 0, p) == _lib.SHELFI_ERR_ARG
    assert lib.shelfi_multi_mult_eval_key(None, p, p) == _lib.SHELFI_ERR_ARG
    assert lib.shelfi_abi_version() == 1


# ---- the helpers tests/test_gpu_multikey_edges.py's sweeps lean on ----
def _planted(x, kind, rng):
    N, q = x["N"], x["q"]
    mods = MK.ext_moduli(N, q)
    dn = x["mid"].shape[1]
    if kind == "full":
        return MK.full_key(mods, dn, N)
    if kind == "zero":
        return np.zeros_like(x["mid"])
    return MK.uniform_key(rng, mods, dn, N)


def test_planted_keys_are_canonical_and_cover_their_range():
    x = _setup("n11_L3_P3")
    N, q = x["N"], x["q"]
    mods = MK.ext_moduli(N, q)
    _, m2, _ = R.s_ext(x["sks"][0], q, x["psi"])
    assert [int(v) for v in mods] == [int(v) for v in m2] and len(mods) == x["mid"].shape[2]
    u = MK.uniform_key(np.random.default_rng(1), mods, 2, N)
    f = MK.full_key(mods, 2, N)
    assert u.shape == f.shape == x["mid"].shape and u.dtype == f.dtype == np.uint64
    assert (u < mods[None, None, :, None]).all() and (f + np.uint64(1) == mods[None, None, :, None]).all()
    # uniform: the top bit of every tower's range is drawn, and no two rows agree
    assert ((u.max(axis=-1) >> np.uint64(1)) >= (mods >> np.uint64(2))[None, None]).all()
    assert len({r.tobytes() for r in u.reshape(-1, N)}) == u.size // N


@pytest.mark.parametrize("cid", ["n11_L3_P3", "n12_L4_30bit_P3"])
@pytest.mark.parametrize("kind", ["full", "zero", "uniform"])
def test_share_from_terms_is_share(cid, kind):
    """share_terms / share_from_terms restate share(..., prev) for any prev, at the EvalMult index and at
    both ends of the rotation range; the share hides the same small error whatever prev holds."""
    x = _setup(cid)
    N, q, psi, sd, sk = x["N"], x["q"], x["psi"], x["seeds"][1], x["sks"][1]
    prev = _planted(x, kind, np.random.default_rng(3))
    for r in (0, 1, -(N // 2 - 1)):
        terms = MK.share_terms(sd, sk, q, psi, r)
        got = MK.share_from_terms(terms, prev)
        assert np.array_equal(got, MK.share(sd, sk, q, psi, r, prev))
        other = prev.copy()
        other[0] = 0  # prev's b-vector is not read
        assert np.array_equal(MK.share_from_terms(terms, other), got)
        e = MK.switch_key_error(got, r, sk, q, psi)
        assert (e == e[:, :1]).all() and 0 < np.abs(e).max() < MK.B_ERR
        assert np.array_equal(e, MK.switch_key_error(MK.share(sd, sk, q, psi, r), r, sk, q, psi))


@pytest.mark.parametrize("cid", ["n11_L3_P3", "n12_L4_30bit_P3"])
@pytest.mark.parametrize("kind", ["full", "zero", "uniform"])
def test_round2_from_terms_is_round2(cid, kind):
    x = _setup(cid)
    q, psi, sd, sk = x["q"], x["psi"], x["seeds"][2], x["sks"][2]
    joint = _planted(x, kind, np.random.default_rng(4))
    terms = MK.round2_terms(sd, sk, q, psi)
    got = MK.round2_from_terms(terms, joint)
    assert np.array_equal(got, MK.round2(sd, joint, sk, q, psi))
    if kind == "zero":
        assert np.array_equal(got, terms[0])


@pytest.mark.parametrize("cid", ["n11_L3_P3", "n12_L4_30bit_P3"])
def test_chain_step_is_a_key_chain(cid):
    """chain_step over the oracle's own lead key: the secret is the oracle's for that seed, a is kept, and
    b + a (s_0 + s_1) is e_0 + e_1 -- small, the same in every tower; over any prev, b - prev.b + a s_1 is
    the seed's e_1."""
    x = _setup(cid)
    N, q, psi = x["N"], x["q"], x["psi"]
    s0, e0, a0 = O.sample_keygen(41, N, q)
    sk0, pk0 = O.keygen(s0, e0, a0, q, psi)
    s1, e1, a1 = O.sample_keygen(42, N, q)
    pk1, sk1 = MK.chain_step(42, pk0, q, psi)
    assert np.array_equal(sk1, O.keygen(s1, e1, a1, q, psi)[0]) and np.array_equal(pk1[1], pk0[1])
    both = MK.sk_sum([sk0, sk1], q)
    mods = MK.ext_moduli(N, q)[:len(q)]
    for t in range(len(q)):
        m = np.uint64(q[t])
        d = (pk1[0, t] + R.mulmod(pk1[1, t], both[t], m)) % m
        assert np.array_equal(O.to_signed(O.ntt_inv(d, q[t], psi[t]), q[t]), e0 + e1)
    rng = np.random.default_rng(6)
    prevs = [np.stack([rng.integers(0, int(m), size=(2, N), dtype=np.uint64) for m in mods], axis=1),
             np.zeros((2, len(q), N), np.uint64), np.broadcast_to((mods - np.uint64(1))[None, :, None],
                                                                  (2, len(q), N)).copy()]
    for prev in prevs:
        pk, sk = MK.chain_step(42, prev, q, psi)
        assert np.array_equal(sk, sk1) and np.array_equal(pk[1], prev[1])
        for t in range(len(q)):
            m = np.uint64(q[t])
            d = (pk[0, t] + (m - prev[0, t]) % m + R.mulmod(prev[1, t], sk[t], m)) % m
            assert np.array_equal(O.to_signed(O.ntt_inv(d, q[t], psi[t]), q[t]), e1)


def test_first_index_with_galois_above():
    N = 1 << 17
    r = MK.first_index_with_galois_above(N, 1 << 17)
    assert r > 0 and R.galois(N, r) > 1 << 17
    assert all(R.galois(N, k) <= 1 << 17 for k in range(1, r))
    assert MK.first_index_with_galois_above(2048, 4) == 1 and MK.first_index_with_galois_above(2048, 5) == 2


def test_sparse_rotation_under_joint_keys():
    """A batch below N / 2 (sparse packing): the joint rotation keys of indices 1 and batch - 1 rotate the
    batch's slots, decrypted under sum s_i."""
    x = _setup("n11_L3_P3")
    N, q, psi, sk = x["N"], x["q"], x["psi"], x["sk"]
    S, d = N // 8, float(q[-1])
    _, rot, _ = MK.protocol(x["seeds"], x["sks"], q, psi, indices=(S - 1,))
    rot[1] = x["rot"][1]
    v = np.random.default_rng(9).uniform(-1, 1, S)
    ct = O.encrypt_vector(v, x["pk"], q, psi, N, S, d, seed=8)
    for r in (1, S - 1):
        dec = O.decrypt_vector(R.rotate_ref(ct, r, rot[r], q, psi), sk, q, psi, S, d, S)
        assert np.abs(dec - np.roll(v, -r)).max() < 1e-6, r
