"""The permutation of a slot rotation alone, on every ring and for many Galois elements.

With c1 = 0 the key switch of sigma_g(c1) is exactly zero whatever key is installed, so
Rotate((c0, 0), r) must be exactly (c0[..., src_g], 0) with src_g = R.gather_index(N, g): one numpy gather,
no oracle key switch (tests/test_rotation_ref.py holds both claims on the CPU).  That makes a sweep of
galois_src (dev_common.h: two __brev and a 32-bit product that wraps from 2^16 on) cost milliseconds an
index: rings 2^11 .. 2^17 at full packing and a sparse one (ring 2^15, batch 4096), 2 towers, K = 2, the
31 indices of R.sweep_indices(batch) each -- both signs, around batch / 2 and batch / 4, the largest, and
sixteen seeded draws.

c0[k][t][j] = (j + N (t + 2 k) + 1) mod q_t: every position of every row carries its own address, so a
misplaced element names where it came from.  One real key (rotationKeyGen([1])) is installed under every
swept index.  `out` is passed in filled with ones: the second component is zero only if the front pass
stores its zeros (the key switch's finish adds into `out`)."""
import functools

import numpy as np
import pytest

import rotation_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

# id: (ring, batch)
RINGS = {"n%d" % l: (1 << l, 1 << (l - 1)) for l in range(11, 18)}
RINGS["n15_sparse"] = (1 << 15, 4096)
K, TOWERS = 2, 2


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@functools.lru_cache(maxsize=None)
def ctx(rid):
    N, batch = RINGS[rid]
    c = m.CKKS("ckks", batch, 52, "", multDepth=TOWERS - 1, firstModBits=60, ringDim=N,
               seed=1100 + list(RINGS).index(rid), decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    assert (inf["ring_dim"], inf["num_towers"], inf["batch"]) == (N, TOWERS, batch)
    q = np.array(inf["moduli"], np.uint64)
    c.rotationKeyGen([1])
    key = c.get_rotation_key(1)
    idx = R.sweep_indices(batch)
    assert len(idx) == 31 and len(set(idx)) == 31 and all(0 < abs(r) < batch for r in idx)
    for r in idx:  # at most 31 Galois elements: within the 64 keys a context holds
        c.set_rotation_key(r, key)
    ct = np.zeros((K, 2, TOWERS, N), np.uint64)
    j = np.arange(N, dtype=np.uint64)
    for k in range(K):
        for t in range(TOWERS):
            ct[k, 0, t] = (j + np.uint64(N * (t + 2 * k) + 1)) % q[t]
    return dict(c=c, N=N, idx=idx, ct_np=ct, ct=_dev(ct))


def test_the_sweep_reaches_both_halves_of_the_galois_range():
    """g above N (the product's top bit) and below 2^16 everywhere; g from 2^16 on, where the 32-bit product
    g e wraps, on the two rings that have such elements."""
    for rid, (N, batch) in RINGS.items():
        gs = [R.galois(N, r) for r in R.sweep_indices(batch)]
        assert any(g > N for g in gs) and any(g < 1 << 16 for g in gs), rid
        if N >= 1 << 16:
            assert sum(g >= 1 << 16 for g in gs) >= 8, rid


@pytest.mark.parametrize("rid", list(RINGS))
def test_rotation_with_a_zero_second_component_is_the_pure_gather(rid):
    x = ctx(rid)
    c, N, ct = x["c"], x["N"], x["ct"]
    out = torch.ones_like(ct)
    for r in x["idx"]:
        out.fill_(1)  # dirty: the zeros of the second component have to be stored
        assert D.rotate(c, ct, r, out=out) is out
        got = _u64(out)
        src = R.gather_index(N, R.galois(N, r))
        bad = np.argwhere(got[:, 0] != x["ct_np"][:, 0][..., src])
        assert not len(bad), "r = %d: first wrong (k, t, j) %s holds %d" % (r, bad[0], got[:, 0][tuple(bad[0])])
        assert not got[:, 1].any(), r


@pytest.mark.parametrize("rid", list(RINGS))
def test_rotation_of_zero_is_zero(rid):
    x = ctx(rid)
    zero = torch.zeros_like(x["ct"])
    for r in x["idx"][:4] + x["idx"][-2:]:
        out = torch.ones_like(zero)
        D.rotate(x["c"], zero, r, out=out)
        assert not out.any(), r
