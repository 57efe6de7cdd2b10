"""The chunk loops of eval.cpp on the MI355X: shelfi_dev_mult, shelfi_dev_rescale,
shelfi_dev_rotate and shelfi_dev_eval_sum split a batch into launch chains whose scratch fits
SHELFI_EVAL_CHUNK_MIB (2048 by default, which no test's batch exceeds: every other test takes one chain).
Here the budget is cut until K = 5 ciphertexts take three chains (2, 2, 1: a ragged last chain, the
scratch laid out again for a smaller kc) and five, CKKS.eval_chunk_count() says that they did, and every
output is bit-identical to the one-chain call and to the reference (the oracle's EvalMult and ModReduce,
tests/rotation_ref.py).  The five ciphertexts all differ and every output buffer starts filled with ones,
so a chain that reads or writes at another k shows.

Context: ring 2^13, 3 towers (tests/test_gpu_rotate.py's n13_L3), dnum 2 / alpha 2 / kP 2.  The scratch per
ciphertext is restated from keyswitch.hip's ks_scratch_bytes and rescale_scratch_bytes; the budgets are
whole MiB (the switch takes positive integers):

  call                      bytes / ciphertext   cap 2 (chains 2, 2, 1)   cap 1 (five chains)
  mult, rotate, 3 towers    29 N 8 = 1.81 MiB    4 MiB                    1 MiB
  eval_sum, 3 towers        + 2 3 N 8: 2.19 MiB  5 MiB                    1 MiB
  rotate, 2 towers          18 N 8 = 1.13 MiB    3 MiB                    1 MiB
  eval_sum, 2 towers        + 2 2 N 8: 1.38 MiB  3 MiB                    1 MiB
  rescale, 3 towers         2 3 N 8 = 0.38 MiB   1 MiB                    none

ModReduce of 3 towers at 2^13 needs 0.38 MiB a ciphertext, so the smallest budget, 1 MiB, already holds
two: no budget gives it a cap of 1 at this shape.  Its five-chain case therefore runs on a ring of 2^15
with 4 towers (2 MiB + 64 bytes a ciphertext: 2 MiB holds one), K = 5, against the oracle alone."""
import functools

import numpy as np
import pytest

import oracle as O
import rotation_ref as R
from conftest import set_switch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

SWITCH = "SHELFI_EVAL_CHUNK_MIB"
K = 5
CHAINS = {2: 3, 1: 5}  # cap (ciphertexts a chain may hold) -> chains of K = 5: (2, 2, 1) and (1, 1, 1, 1, 1)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _ks_bytes(N, Ll, alpha, kP):
    """keyswitch.hip ks_scratch_bytes for one ciphertext: d2e | d2c | ext | accQ | accP | z."""
    T, dn = Ll + kP, -(-Ll // alpha)
    ext = sum(T - min(alpha, Ll - j * alpha) for j in range(dn))
    return N * 8 * (2 * Ll + ext + 2 * Ll + 2 * kP + 2 * Ll) + 64


def _rescale_bytes(N, Ll):
    """keyswitch.hip rescale_scratch_bytes for one ciphertext: the last tower | v."""
    return 2 * N * 8 * (1 + (Ll - 1)) + 64


def _budget(per_ct, cap):
    """The whole-MiB budget under which eval.cpp's chunk_of caps a chain at `cap` ciphertexts
    (cap = max(1, budget / per_ct)); None if there is none."""
    for mib in range(1, 64):
        if max(1, (mib << 20) // per_ct) == cap:
            return str(mib)
    return None


@functools.lru_cache(maxsize=None)
def ctx(N=1 << 13, depth=2):
    """One context for the module: every key the calls need, five different ciphertexts."""
    c = m.CKKS("ckks", N // 2, 52, "", multDepth=depth, firstModBits=60, ringDim=N, seed=811, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    S = inf["batch"]
    assert (inf["ring_dim"], inf["num_towers"], S) == (N, depth + 1, N // 2)
    q, psi = np.array(inf["moduli"], np.uint64), np.array(inf["roots"], np.uint64)
    dn, al, p, _ = O.special_primes(N, q)
    x = np.random.default_rng(811).uniform(-1, 1, K * S)
    ct = D.encrypt(c, torch.tensor(x, dtype=torch.float64, device="cuda"))
    assert ct.shape == (K, 2, depth + 1, N)
    ct_np = _u64(ct)
    assert len({ct_np[k].tobytes() for k in range(K)}) == K
    return dict(c=c, N=N, S=S, q=q, psi=psi, alpha=al, kP=len(p), ct=ct, ct_np=ct_np, keys={}, refs={})


def _keys(x):
    if not x["keys"]:
        c = x["c"]
        c.evalMultKeyGen()
        c.evalSumKeyGen()
        c.rotationKeyGen([-2])
        x["evk"] = c.get_eval_key()
        x["keys"] = {r: c.get_rotation_key(r) for r in [-2] + [1 << i for i in range(x["S"].bit_length() - 1)]}
    return x


def _input(x, towers):
    ct = x["ct"] if towers == x["ct"].shape[2] else x["ct"][:, :, :towers].contiguous()
    return ct, x["ct_np"][:, :, :towers]


# name -> (call on the device into `out`, reference, scratch bytes a ciphertext)
def _ops(x):
    N, al, kP, q, psi = x["N"], x["alpha"], x["kP"], x["q"], x["psi"]
    c = x["c"]

    def ks(t):
        return _ks_bytes(N, t, al, kP)

    def esum(n):
        return (lambda ct, out: D.eval_sum(c, ct, n, out=out), lambda a: R.eval_sum_ref(a, n, x["keys"], q, psi),
                lambda t: ks(t) + 2 * t * N * 8)

    return {
        # the second operand is the batch reversed: a chain that pairs a[k] with another b shows
        "mult": (lambda ct, out: D.mult(c, ct, ct.flip(0).contiguous(), out=out),
                 lambda a: O.eval_mult(a, np.ascontiguousarray(a[::-1]), x["evk"], q, psi), ks),
        "rescale": (lambda ct, out: D.rescale(c, ct, out=out), lambda a: O.rescale(np.ascontiguousarray(a), q, psi),
                    lambda t: _rescale_bytes(N, t)),
        "rotate": (lambda ct, out: D.rotate(c, ct, -2, out=out),
                   lambda a: R.rotate_ref(a, -2, x["keys"][-2], q, psi), ks),
        "eval_sum_4": esum(4),
        "eval_sum_batch": esum(x["S"]),
    }


def _dirty(ct, rescale=False):
    """An output buffer of ones.  A fresh torch.empty is usually the block the previous call's result
    was freed from, still holding the right answer: a chain that writes nowhere, or at another
    ciphertext, would go unseen."""
    K, _, l, N = ct.shape
    return torch.ones((K, 2, l - 1 if rescale else l, N), dtype=ct.dtype, device=ct.device)


def _reference(x, op, towers):
    """Computed once for both budgets, never written to."""
    if (op, towers) not in x["refs"]:
        ref = _ops(x)[op][1](_input(x, towers)[1])
        ref.setflags(write=False)
        x["refs"][(op, towers)] = ref
    return x["refs"][(op, towers)]


CASES = [(op, 3, cap) for op in ("mult", "rotate", "eval_sum_4", "eval_sum_batch") for cap in (2, 1)]
CASES += [("rescale", 3, 2)]  # cap 1: test_rescale_in_five_chains
# a level below the top: the partial digit (dn = 1 of the chain's 2), a ciphertext stride below the context's
CASES += [(op, 2, cap) for op in ("rotate", "eval_sum_4") for cap in (2, 1)]


@pytest.mark.parametrize("op,towers,cap", CASES)
def test_chunked_call_is_counted_and_bit_identical(monkeypatch, op, towers, cap):
    x = _keys(ctx())
    c = x["c"]
    call, _, per_ct = _ops(x)[op]
    ct = _input(x, towers)[0]
    mib = _budget(per_ct(towers), cap)
    assert mib is not None, "no whole-MiB budget caps %s at %d: %d bytes a ciphertext" % (op, cap, per_ct(towers))
    set_switch(monkeypatch, SWITCH, None)
    whole = _u64(call(ct, _dirty(ct, op == "rescale")))
    assert c.eval_chunk_count() == 1
    set_switch(monkeypatch, SWITCH, mib)
    got = _u64(call(ct, _dirty(ct, op == "rescale")))
    print("%s at %d towers, %s MiB: %d chains" % (op, towers, mib, c.eval_chunk_count()))
    assert c.eval_chunk_count() == CHAINS[cap]
    assert np.array_equal(got, whole)
    assert np.array_equal(got, _reference(x, op, towers))


def test_rescale_in_five_chains(monkeypatch):
    """ModReduce one ciphertext a chain (the input stride 2 l N against the output's 2 (l - 1) N, five
    times): ring 2^15, 4 towers, where a ciphertext's scratch is just above 2 MiB (see the module's note)."""
    x = ctx(1 << 15, 3)
    c, ct = x["c"], x["ct"]
    mib = _budget(_rescale_bytes(x["N"], 4), 1)
    assert mib is not None
    set_switch(monkeypatch, SWITCH, None)
    whole = _u64(D.rescale(c, ct, out=_dirty(ct, True)))
    assert c.eval_chunk_count() == 1
    set_switch(monkeypatch, SWITCH, mib)
    got = _u64(D.rescale(c, ct, out=_dirty(ct, True)))
    assert c.eval_chunk_count() == 5
    assert np.array_equal(got, whole)
    assert np.array_equal(got, O.rescale(x["ct_np"], x["q"], x["psi"]))


def test_counter_of_calls_that_enqueue_nothing_and_of_refused_calls(monkeypatch):
    x = _keys(ctx())
    c, ct, N = x["c"], x["ct"], x["N"]
    set_switch(monkeypatch, SWITCH, _budget(_ks_bytes(N, 3, x["alpha"], x["kP"]), 1))
    D.rotate(c, ct, -2)
    assert c.eval_chunk_count() == 5
    with pytest.raises(RuntimeError, match="rotation key"):  # refused: the counter keeps the last call's
        D.rotate(c, ct, 3)
    with pytest.raises(ValueError, match="overlap"):
        D.rotate(c, ct, -2, out=ct)
    with pytest.raises(ValueError):
        D.eval_sum(c, ct, 3)
    assert c.eval_chunk_count() == 5
    assert torch.equal(D.rotate(c, ct, 0), ct) and c.eval_chunk_count() == 0  # a copy
    D.mult(c, ct[:1], ct[:1])
    assert c.eval_chunk_count() == 1
    assert torch.equal(D.eval_sum(c, ct, 1), ct) and c.eval_chunk_count() == 0  # a copy
    lib = _lib.load()
    for call in (lambda: lib.shelfi_dev_rotate(c._ctx, None, 0, 3, -2, None, None),
                 lambda: lib.shelfi_dev_eval_sum(c._ctx, None, 0, 3, 4, None, None),
                 lambda: lib.shelfi_dev_mult(c._ctx, None, None, 0, 3, None, None),
                 lambda: lib.shelfi_dev_rescale(c._ctx, None, 0, 3, None, None)):
        D.rotate(c, ct[:2], -2)
        assert c.eval_chunk_count() == 2
        assert call() == 0 and c.eval_chunk_count() == 0  # K = 0


def test_guards_and_exact_alias_under_a_one_ciphertext_budget(monkeypatch):
    """The overlap checks cover the whole batch, not one chain; and the alias the product allows (out is
    a) still gives the reference: a chain writes its own ciphertexts only."""
    x = _keys(ctx())
    c, ct, N = x["c"], x["ct"], x["N"]
    per = _ks_bytes(N, 3, x["alpha"], x["kP"])
    set_switch(monkeypatch, SWITCH, _budget(per + 2 * 3 * N * 8, 1))
    assert _budget(per, 1) is not None and max(1, (1 << 20) // per) == 1
    flat = torch.zeros(ct.numel() + N, dtype=ct.dtype, device="cuda")
    shifted, out = flat[N:].view(ct.shape), flat[:ct.numel()].view(ct.shape)
    with pytest.raises(ValueError, match="overlap"):
        D.rotate(c, shifted, -2, out=out)
    with pytest.raises(ValueError, match="overlap"):
        D.eval_sum(c, shifted, 4, out=out)
    with pytest.raises(ValueError, match="overlap"):
        D.mult(c, shifted, ct, out=out)
    with pytest.raises(ValueError, match="overlap"):
        D.mult(c, ct, shifted, out=out)
    a, b = ct.clone(), ct.flip(0).contiguous()
    assert D.mult(c, a, b, out=a) is a
    assert c.eval_chunk_count() == 5
    assert np.array_equal(_u64(a), _reference(x, "mult", 3)) and np.array_equal(_u64(b), x["ct_np"][::-1])
