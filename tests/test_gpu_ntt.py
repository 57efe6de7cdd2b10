"""The standalone NTT on the MI355X (shelfi_dev_ntt / device.ntt = launch_ntt, csrc/ntt.hip) against the
oracle, bit for bit, on tests/ntt_cases.py: every ring 2^10 .. 2^17, every modulus class (60/52-bit
red_ok towers, 45/42/41-bit, and the 60/31- and 40/31-bit chains that take the run-time-shape block
kernels), the forward and the inverse each on its own, on uniform, extreme and sparse-output inputs
(tests/test_ntt_cases.py holds the oracle to the definition on the CPU).  Then the batch shapes
(P = 1, P not a multiple of L, P = 0, a null pointer), a non-default stream, device.ntt's guard, and
SHELFI_NTT_BLOCK_LOG_BIG = 11 / 12 in child processes: 11 at ring 2^17 is the only way to the
6-stage, 64-row column passes (ntt_fwd_cols<6>, ntt_inv_cols<6>, plain_cols<6> and the `case 6:`
launches of encrypt, decrypt, the key switch and the partial decryption)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ntt_cases as NC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import _lib  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
BATCH_SHAPES = ("2^15/L4", "2^16/60-31bit")
IN_CHILD = os.environ.get("SHELFI_NTT_BLOCK_LOG_BIG") is not None


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).cuda()  # a copy: the call is in place


@functools.lru_cache(maxsize=None)
def bare(name):
    """A keyless context of a shape; its chain is the oracle's."""
    batch, _, _, sb, _ = NC.SHAPES[name]
    ck = m.CKKS("ckks", batch, sb, "", seed=9, decodeNoise=False, **NC.ckks_kwargs(name))
    ch = NC.chain(name)
    inf = ck.info()
    assert not inf["keys_loaded"]
    assert (inf["ring_dim"], inf["batch"], inf["num_towers"]) == (ch.N, ch.S, ch.L)
    assert np.array_equal(np.array(inf["moduli"], np.uint64), ch.q)
    assert np.array_equal(np.array(inf["roots"], np.uint64), ch.psi)
    return ck, ch


def _ntt(ck, a, inverse):
    t = _dev(a)
    assert D.ntt(ck, t, inverse=inverse) is t
    torch.cuda.synchronize()
    return _u64(t)


# ------------------------------------------------- 1. each direction against the oracle ----
@pytest.mark.parametrize("name", list(NC.SHAPES))
def test_forward_and_inverse_bitexact(name):
    ck, ch = bare(name)
    for inverse in (False, True):
        x, want, rows = NC.batch(name, inverse)
        got = _ntt(ck, x, inverse)
        assert NC.first_difference(got, want, rows) is None, \
            (name, "inverse" if inverse else "forward") + NC.first_difference(got, want, rows)
        back = _ntt(ck, got, not inverse)
        assert NC.first_difference(back, x, rows) is None, \
            (name, "round trip from", "inverse" if inverse else "forward") + NC.first_difference(back, x, rows)


# ------------------------------------------------------------------ 2. batch shapes ----
def _rows_for(name, inverse, P):
    """P polynomials, polynomial p on tower p % L: the uniform class first, then the sparse one."""
    ch = NC.chain(name)
    x, want, rows = NC.batch(name, inverse)
    order = ("uniform", "sparse", "full", "halves_lo")
    pick = [rows.index((order[p // ch.L], p % ch.L)) for p in range(P)]
    return x[pick], want[pick], [rows[i] for i in pick]


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("name", BATCH_SHAPES)
def test_any_polynomial_count(name, inverse):
    ck, ch = bare(name)
    for P in (1, ch.L + 1, 2 * ch.L - 1):
        x, want, rows = _rows_for(name, inverse, P)
        assert x.shape == (P, ch.N) and [t for _, t in rows] == [p % ch.L for p in range(P)]
        got = _ntt(ck, x, inverse)
        assert NC.first_difference(got, want, rows) is None, (P,) + NC.first_difference(got, want, rows)


@pytest.mark.parametrize("name", BATCH_SHAPES)
def test_empty_call_and_null_pointer(name):
    ck, ch = bare(name)
    lib = _lib.load()
    x, _, _ = _rows_for(name, False, ch.L)
    t = _dev(x)
    for inverse in (0, 1):
        assert lib.shelfi_dev_ntt(ck._ctx, None, 0, inverse, None) == 0
        assert lib.shelfi_dev_ntt(ck._ctx, C.c_void_p(t.data_ptr()), 0, inverse, None) == 0
        for P in (1, ch.L):
            assert lib.shelfi_dev_ntt(ck._ctx, None, P, inverse, None) == _lib.SHELFI_ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(_u64(t), x)
    # the context still works
    x1, want, rows = _rows_for(name, False, ch.L)
    assert NC.first_difference(_ntt(ck, x1, False), want, rows) is None


# ----------------------------------------------------------- 3. a non-default stream ----
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("name", BATCH_SHAPES)
def test_non_default_stream(name, inverse):
    ck, ch = bare(name)
    x, want, rows = _rows_for(name, inverse, 2 * ch.L - 1)
    default = _ntt(ck, x, inverse)
    s = torch.cuda.Stream()
    t = _dev(x)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        D.ntt(ck, t, inverse=inverse)
    s.synchronize()
    got = _u64(t)
    assert np.array_equal(got, default)
    assert NC.first_difference(got, want, rows) is None, NC.first_difference(got, want, rows)


# ------------------------------------------------------------------ 4. Python guard ----
def test_guard_refuses_other_dtypes_and_sizes():
    """int32 / float32 [P][N] is half the bytes of P polynomials: refused before any launch."""
    ck, ch = bare("2^13/L2")
    N, sentinel = ch.N, 0x5A
    refused = [torch.empty((2, N), dtype=dt, device="cuda")
               for dt in (torch.int32, torch.float32, torch.float64, torch.int16, torch.uint8, torch.float16)]
    refused += [torch.empty(shape, dtype=torch.int64, device="cuda")
                for shape in ((2, N + 1), (2, N - 1), (N // 2,), (3, N // 2), (2 * N + 5,))]
    for t in refused:
        raw = t.view(torch.uint8)
        raw.fill_(sentinel)
        for inverse in (False, True):
            with pytest.raises(ValueError):
                D.ntt(ck, t, inverse=inverse)
        torch.cuda.synchronize()
        assert bool((raw == sentinel).all()), (t.dtype, tuple(t.shape))
    with pytest.raises(ValueError):
        D.ntt(ck, torch.zeros((2, N), dtype=torch.int64))  # a host tensor
    with pytest.raises(ValueError):
        D.ntt(ck, torch.zeros((N, 2), dtype=torch.int64, device="cuda").t())  # not contiguous
    # int64 of any leading shape is taken
    x, want, rows = NC.batch("2^13/L2", False)
    t = _dev(x[:4]).view(2, 2, N)
    D.ntt(ck, t)
    torch.cuda.synchronize()
    assert NC.first_difference(_u64(t).reshape(4, N), want[:4], rows[:4]) is None


# ------------------------------------------- 5. the other block sizes, in child processes ----
# Time limit of a child: test_gpu_shapes.py::test_large_rings_with_2p12_blocks (a child of the same
# kind, 5 tests) took 6.7 s on an MI355X; beside it, the 2^11-blocks child here (22 tests) took 12.8 s
# and the 2^12-blocks one (7 tests) 4.2 s.  40 times the base, rounded up to 7 s.
CHILD_BASE_S = 7
CHILD_TIMEOUT_S = 40 * CHILD_BASE_S


def _child(block_log, selections):
    """One pytest in a fresh process with SHELFI_NTT_BLOCK_LOG_BIG set (read once per process) over
    (file, -k expression) selections; every file must have a test that ran and passed."""
    env = dict(os.environ, SHELFI_NTT_BLOCK_LOG_BIG=str(block_log))
    expr = " or ".join("(%s and (%s))" % (os.path.splitext(f)[0], e) for f, e in selections)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-rp", "-p", "no:cacheprovider", "-m", "gpu"]
                       + [os.path.join(HERE, f) for f, _ in selections] + ["-k", expr],
                       env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " passed" in r.stdout and " failed" not in r.stdout, r.stdout[-3000:]
    passed = [ln for ln in r.stdout.splitlines() if ln.startswith("PASSED")]
    for f, e in selections:
        assert any(f + "::" in ln for ln in passed), (f, e, r.stdout[-3000:])
    return passed


@pytest.mark.skipif(IN_CHILD, reason="already the child")
def test_ring_2p17_with_2p11_blocks():
    """logN - BL = 6: the 64-row column passes of the NTT, encode, encrypt, decrypt, the key switch
    (EvalMult, rotations) and the partial decryption."""
    _child(11, [
        ("test_gpu_ntt.py", "17/"),
        ("test_gpu_shapes.py", "bitexact and 65536-0"),
        ("test_gpu_plain_ops.py", "test_encode_bitexact_on_every_shape and 17/L2"),
        ("test_gpu_f4.py", "b65536_d1_s52"),
        ("test_gpu_rotate.py", "n17_L2"),
        ("test_gpu_threshold.py", "b65536_d1_s52"),
    ])


@pytest.mark.skipif(IN_CHILD, reason="already the child")
def test_ring_2p16_with_2p12_blocks():
    """4 column stages over 2^12 blocks, at compile-time and at run-time shape."""
    passed = _child(12, [("test_gpu_ntt.py", "16/")])
    assert sum("test_forward_and_inverse_bitexact" in ln for ln in passed) == 2
