"""The smudging-noise stream of the threshold partial decryption (DESIGN.md §2.10 "Noise stream",
threshold.hip's header comment): the C oracle's or_threshold_noise against an independent pure-Python
restatement on top of the RFC 8439-checked ChaCha20 block (test_oracle_kat.py), as test_sampler_v2.py does
for encrypt's sampler.

The two are written in opposite directions -- the C function walks the stream's blocks and scatters their
normals, the restatement below walks the coefficients and looks each one's (block, normal) up -- so an index
slip in either shows as a difference.  Both evaluate Box-Muller in binary64 through the same libm, so the
integers are equal, not close.  The GPU kernels are compared with this oracle in
test_gpu_threshold_stream.py.

Also checked here, on the restatement's own index map: no (block, normal) pair serves two coefficients of a
polynomial (repeated noise inside a polynomial is what weakens smudging), ciphertexts g and g + 1 share no
block, and the oracle's integers meet the statistics bounds test_gpu_threshold.py applies to the device's."""
import math

import numpy as np
import pytest

import oracle as O

NONCE = 5 << 56
# logN -> rows R of the columns pass: 4: one block (R = 1), 11: the largest single block, 12 / 14: R = 2 / 8
# (a column's block partly used), 16: R = 32 on 2^11 blocks, 17: R = 32 on 2^12 blocks (both nb = 2)
LOGNS = [4, 11, 12, 14, 16, 17]


def _block_log(logN):
    return 12 if logN == 17 else min(logN, 11)


def _slot(j, logN, bl):
    """(block, normal) of coefficient j."""
    rows = 1 << (logN - bl)
    if rows == 1:
        return j >> 4, j & 15
    row, col = j >> bl, j & ((1 << bl) - 1)
    nb = max(1, rows // 16)
    return col * nb + (row >> 4), row & 15


def _py_noise(seed, g, logN, sigma):
    key = O.seed_to_key(seed)
    bl = _block_log(logN)
    cache = {}

    def normals(b):
        if b not in cache:
            w = [int(x) for x in O.chacha20_block(key, b, NONCE | g)]
            z = []
            for u in range(8):
                lo, hi = w[2 * u], w[2 * u + 1]
                r = math.sqrt(-2.0 * math.log((lo + 1) * 2.0 ** -32))
                a = 2.0 * math.pi * (hi * 2.0 ** -32)
                z += [r * math.cos(a), r * math.sin(a)]
            cache[b] = z
        return cache[b]

    e = np.zeros(1 << logN, np.int64)
    for j in range(1 << logN):
        b, n = _slot(j, logN, bl)
        x = sigma * normals(b)[n]
        t = math.trunc(x)
        if abs(x - t) >= 0.5:  # ties away from zero
            t += 1 if x > 0 else -1
        e[j] = t
    return e


def test_block_log_rule():
    for logN in range(4, 18):
        assert O.threshold_block_log(logN) == _block_log(logN)


@pytest.mark.parametrize("logN", LOGNS)
@pytest.mark.parametrize("sigma", [2.0 ** 20, 3.19], ids=["s2p20", "s3.19"])
def test_oracle_noise_matches_python_restatement(logN, sigma):
    g = 3 + logN
    got = O.threshold_noise(9, g, 1 << logN, _block_log(logN), sigma)
    assert np.array_equal(got, _py_noise(9, g, logN, sigma))
    assert np.array_equal(got, O.threshold_noise(9, g, 1 << logN, sigma=sigma))  # the default block size
    assert not np.array_equal(got, O.threshold_noise(9, g + 1, 1 << logN, sigma=sigma))
    assert not np.array_equal(got, O.threshold_noise(10, g, 1 << logN, sigma=sigma))


@pytest.mark.parametrize("logN", list(range(4, 18)))
def test_no_normal_serves_two_coefficients(logN):
    bl = _block_log(logN)
    j = np.arange(1 << logN, dtype=np.int64)
    rows = 1 << (logN - bl)
    if rows == 1:
        blk, nrm = j >> 4, j & 15
    else:
        row, col = j >> bl, j & ((1 << bl) - 1)
        blk, nrm = col * max(1, rows // 16) + (row >> 4), row & 15
    for jj in (0, 1, 15, (1 << logN) - 1, (1 << logN) // 2 + 5):  # the vector form is _slot
        assert (int(blk[jj]), int(nrm[jj])) == _slot(jj, logN, bl)
    assert len(np.unique(blk * 16 + nrm)) == 1 << logN
    # the blocks are 0 .. nblocks - 1 without a gap, each giving min(16, rows) normals (16 when rows = 1)
    per = 16 if rows == 1 else min(16, rows)
    counts = np.bincount(blk)
    assert len(counts) * per == 1 << logN and (counts == per).all()


@pytest.mark.parametrize("logN", [4, 12, 16])
def test_consecutive_ciphertexts_share_no_block(logN):
    """g enters the nonce alone and stays below 2^56, so (nonce, counter) pairs of g and g + 1 are disjoint;
    shown on the stream itself: no block of g + 1 (16 words) equals a block of g, and no oracle integer run
    repeats."""
    key = O.seed_to_key(21)
    nblocks = (1 << logN) // 16 if logN <= 11 else (1 << 11) * max(1, (1 << (logN - 11)) // 16)
    for g in (0, 7, 2 ** 32 - 1):
        assert (NONCE | g) != (NONCE | (g + 1)) and (NONCE | (g + 1)) >> 56 == 5
        a = {tuple(O.chacha20_block(key, b, NONCE | g)) for b in range(min(nblocks, 256))}
        b = {tuple(O.chacha20_block(key, b, NONCE | (g + 1))) for b in range(min(nblocks, 256))}
        assert len(a) == len(b) == min(nblocks, 256) and not (a & b)
    e0 = O.threshold_noise(21, 0, 1 << logN)
    e1 = O.threshold_noise(21, 1, 1 << logN)
    assert np.count_nonzero(e0 == e1) <= 4  # sigma = 2^20: equal integers by chance ~ N 2^-21 each


@pytest.mark.parametrize("sigma", [2.0 ** 20, 3.19], ids=["s2p20", "s3.19"])
def test_oracle_noise_statistics(sigma):
    """test_gpu_threshold.py's bounds, at its 2^15 shape (K = 2 ciphertexts of a call)."""
    e = np.stack([O.threshold_noise(77, g, 1 << 15, sigma=sigma) for g in (0, 1)])
    cnt = e.size
    print("sigma %g: mean %.4g std %.6g max %.4g over %d" % (sigma, e.mean(), e.std(), np.abs(e).max(), cnt))
    assert abs(e.mean()) <= 5 * sigma / np.sqrt(cnt)
    assert abs(e.std() / sigma - 1) <= 0.05
    assert np.abs(e).max() <= 9 * sigma
    assert not np.array_equal(e[0], e[1])
