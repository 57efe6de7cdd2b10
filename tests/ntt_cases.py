"""Inputs that pin the standalone negacyclic NTT (launch_ntt, fhe-fed_amd/csrc/ntt.hip) on every ring,
modulus class and boundary value, for tests/test_ntt_cases.py (CPU: the oracle held to the definition,
every builder lands where it claims) and tests/test_gpu_ntt.py (the HIP kernels against the oracle).

A shape is (batch, ringDim, multDepth, scaleBits, firstModBits), one keyless context each.  For a tower
(q, psi, N) every class is a list of (name, input, expected) per direction, expected always
oracle.ntt_fwd / oracle.ntt_inv of the input:
  uniform      seeded residues below q
  zero         all zeros in, all zeros out (never q)
  full         every coefficient q - 1
  halves_lo/hi q - 1 in one half, 0 in the other: the first stage pairs (max, 0) and (0, max)
  parity_ev/od q - 1 at the even (odd) indices, 0 at the others: the last stage's pairs
  sparse       the input is the oracle's OPPOSITE transform of a target s that is zero except at 8
               positions, so the expected output is s itself: all but 8 outputs are 0, reached in the
               kernel through a lazy value that is an exact multiple of q (0, q, 2q, ... below the
               pass's bound), where a reduction with > for >=, a quotient estimate off by one or a
               skipped conditional subtraction stores q (or a multiple) instead of 0.
"""
import collections
import functools
import os

import numpy as np

import encode_edge_inputs as E
import oracle as O

REUSED = ("2^11/L2", "2^12/L2", "2^13/L2", "2^14/L3", "2^15/L4", "2^16/L2", "2^17/L2",
          "30-bit", "41-bit/2^13", "41-bit/2^15")
SHAPES = collections.OrderedDict([(n, E.SHAPES[n]) for n in REUSED] + [
    ("2^10/L2", (512, 1024, 1, 52, 60)),             # validate_params' minimum: one 2^10 block, stages 3,3,3,1
    ("2^16/60-31bit", (32768, 65536, 1, 30, 60)),    # the run-time-shape kernels, 5 column stages, 8q near 2^63
    ("2^17/40-31bit", (65536, 131072, 1, 30, 40)),   # the run-time-shape kernels on 2^12 blocks (32 KiB of LDS)
    ("2^13/L1", (4096, 8192, 0, 52, 60)),            # one tower: every polynomial of a call uses it
])
# the oracle's bit lengths of the chains that are chosen for them
BITS = {"2^10/L2": [60, 53], "2^16/60-31bit": [60, 31], "2^17/40-31bit": [40, 31], "2^13/L1": [53],
        "30-bit": [40, 31], "41-bit/2^13": [45, 42], "41-bit/2^15": [45, 42, 41, 42]}

CLASSES = ("uniform", "zero", "full", "halves_lo", "halves_hi", "parity_ev", "parity_od", "sparse")

Chain = collections.namedtuple("Chain", "N S L q psi")


@functools.lru_cache(maxsize=None)
def chain(name):
    """The oracle's parameters of a shape (the product's are checked against them on the GPU)."""
    batch, N, depth, sb, fb = SHAPES[name]
    q, psi = O.params_generate(N, depth + 1, sb, fb)
    return Chain(N, batch, depth + 1, q, psi)


def ckks_kwargs(name):
    """Keyword arguments of SHELFI_FHE.CKKS("ckks", batch, scaleBits, "", ...) for a shape."""
    batch, N, depth, sb, fb = SHAPES[name]
    return dict(multDepth=depth, firstModBits=fb, ringDim=N)


def block_log(N):
    """log2 of the ring's NTT block (ntt_block_log, shelfi_internal.h): 2^11, 2^12 from ring 2^17, the
    whole ring below that; SHELFI_NTT_BLOCK_LOG_BIG = 11 | 12 replaces it from ring 2^16 up."""
    logN = N.bit_length() - 1
    b = 12 if logN >= 17 else 11
    ovr = os.environ.get("SHELFI_NTT_BLOCK_LOG_BIG", "")
    if ovr in ("11", "12") and logN >= 16:
        b = int(ovr)
    return min(b, logN)


def _const(N, v):
    return np.full(N, v, np.uint64)


def sparse_target(q, N, seed):
    """The target s: 8 distinct positions (0, N - 1, both sides of the first block boundary where the
    ring has one, the rest seeded) holding 1, q - 1, (q - 1) / 2, (q + 1) / 2 and seeded non-zero
    residues, in a seeded order; zero elsewhere."""
    rng = np.random.default_rng(seed)
    pos = [0, N - 1]
    B = 1 << block_log(N)
    if B < N:
        pos += [B - 1, B]
    while len(pos) < 8:
        p = int(rng.integers(1, N - 1))
        if p not in pos:
            pos.append(p)
    vals = [1, q - 1, (q - 1) // 2, (q + 1) // 2] + [int(v) for v in rng.integers(1, q, 4, dtype=np.uint64)]
    s = np.zeros(N, np.uint64)
    for p, k in zip(pos, rng.permutation(8)):
        s[p] = vals[k]
    return s, sorted(pos), sorted(vals)


def tower_inputs(q, psi, N, inverse, seed):
    """[(class, input, expected)] of one tower in one direction, in CLASSES' order."""
    q, psi = int(q), int(psi)
    do, undo = (O.ntt_inv, O.ntt_fwd) if inverse else (O.ntt_fwd, O.ntt_inv)
    top = q - 1
    idx = np.arange(N)
    ins = collections.OrderedDict()
    ins["uniform"] = np.random.default_rng(seed).integers(0, q, N, dtype=np.uint64)
    ins["zero"] = _const(N, 0)
    ins["full"] = _const(N, top)
    ins["halves_lo"] = np.where(idx < N // 2, top, 0).astype(np.uint64)
    ins["halves_hi"] = np.where(idx >= N // 2, top, 0).astype(np.uint64)
    ins["parity_ev"] = np.where(idx % 2 == 0, top, 0).astype(np.uint64)
    ins["parity_od"] = np.where(idx % 2 == 1, top, 0).astype(np.uint64)
    out = [(c, a, do(a, q, psi)) for c, a in ins.items()]
    s, _, _ = sparse_target(q, N, seed + 1)
    out.append(("sparse", undo(s, q, psi), s))
    assert tuple(c for c, _, _ in out) == CLASSES
    return out


def _seed(name, t, inverse):
    return 7919 * list(SHAPES).index(name) + 97 * t + (50 if inverse else 0)


@functools.lru_cache(maxsize=None)
def batch(name, inverse):
    """One direction's call of a shape: inputs and expectations [C * L][N] with polynomial p = c L + t
    of class c on tower t = p % L (the tower launch_ntt gives polynomial p), and the (class, tower) of
    every row.  Read-only arrays, shared by the tests."""
    ch = chain(name)
    per = [tower_inputs(ch.q[t], ch.psi[t], ch.N, inverse, _seed(name, t, inverse)) for t in range(ch.L)]
    rows = [(c, t) for c in range(len(CLASSES)) for t in range(ch.L)]
    x = np.stack([per[t][c][1] for c, t in rows])
    want = np.stack([per[t][c][2] for c, t in rows])
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want, [(CLASSES[c], t) for c, t in rows]


def first_difference(got, want, rows):
    """None when equal, else the first differing (class, tower, index, got, want)."""
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    p, i = (int(v) for v in bad[0])
    return rows[p] + (i, int(got[p, i]), int(want[p, i]))
