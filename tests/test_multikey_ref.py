"""tests/multikey_ref.py held to its meaning on the CPU: its restated sampler
reproduces the oracle's EvalMult key draw; the keys its protocol makes hide one small integer
polynomial per digit, the same in every tower of Q u P and below the worst-case bound; and the
oracle's EvalMult / ModReduce and the rotation reference under those keys decode under sum s_i to
x^2, its roll and its windowed sum.  And, with no device: the library exports the three entry points
and they refuse a NULL context."""
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
