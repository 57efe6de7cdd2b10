"""Device-resident batch API over torch tensors (HBM in, HBM out).

PyTorch is used only as plumbing — HBM allocation, the current HIP stream and
torch.distributed (RCCL over xGMI) — while every arithmetic step is a libshelfi
kernel launched on torch's current stream.  Ciphertext batches are uint64 data
in the [K][2][L][N] layout (stored in int64 tensors: torch has no full uint64
arithmetic, and none is done on them here).
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

from . import _lib
from ._lib import check


def _torch():
    import torch  # deferred: the bytes API does not need torch

    return torch


def _stream_ptr(tensor) -> int:
    torch = _torch()
    return torch.cuda.current_stream(tensor.device).cuda_stream


def ct_shape(ckks, K: int):
    inf = ckks.info()
    return (K, 2, inf["num_towers"], inf["ring_dim"])


def empty_ct(ckks, K: int, device=None):
    torch = _torch()
    if device is None:
        device = "cuda:%d" % ckks.info()["device"]
    return torch.empty(ct_shape(ckks, K), dtype=torch.int64, device=device)


def _ln(ckks):
    """(L, N) of a context, cached (info() is a library call and a dict build, too slow for
    the per-launch path of small aggregations).  The cache is keyed on the context's
    parameter generation: loadCryptoParams / genCryptoContextAndKeyGen can change N and L
    (PALISADE files carry their own ring), and bump it (SHELFI_FHE.CKKS._params_gen)."""
    gen = getattr(ckks, "_params_gen", 0)
    ln = getattr(ckks, "_dev_ln", None)
    if ln is None or ln[0] != gen:
        inf = ckks.info()
        ln = ckks._dev_ln = (gen, inf["num_towers"], inf["ring_dim"])
    return ln[1], ln[2]


def _check_ct(t, ckks, K=None, any_level=False):
    # on the per-launch path of small aggregations (cfg2: 17 tensors per ~23 us launch): each tensor
    # attribute is a call into torch, so the shape is read once
    L, N = _ln(ckks)
    if not t.is_cuda or not t.is_contiguous() or t.element_size() != 8:
        raise ValueError("ciphertext tensors must be contiguous 64-bit CUDA tensors")
    sh = t.shape
    if len(sh) != 4 or sh[1] != 2 or sh[3] != N or not ((1 <= sh[2] <= L) if any_level else sh[2] == L):
        raise ValueError("ciphertext tensor must have shape [K][2][L][N] = [K][2][%d][%d]" % (L, N))
    if K is not None and sh[0] != K:
        raise ValueError("ciphertext tensors hold different numbers of ciphertexts")


def wavg(ckks, cts: Sequence, weights: Sequence[float], out=None):
    """sum_c W_c * cts[c] (EvalMult by (float)w_c + EvalAdd), fully on device."""
    torch = _torch()
    cts = list(cts)
    if len(cts) != len(weights) or not cts:
        raise ValueError("need one weight per learner and at least one learner")
    K = cts[0].shape[0]
    for t in cts:
        _check_ct(t, ckks, K)
    if out is None:
        out = torch.empty_like(cts[0])
    _check_ct(out, ckks, K)
    ptrs = (C.c_void_p * len(cts))(*[t.data_ptr() for t in cts])
    w = (C.c_float * len(cts))(*[float(x) for x in weights])
    check(_lib.load().shelfi_dev_wavg(ckks._ctx, ptrs, w, len(cts), K, C.c_void_p(out.data_ptr()),
                                      C.c_void_p(_stream_ptr(out))), "dev_wavg")
    return out


class Arena:
    """The aggregator's resident layout for C learners' K ciphertexts: one HBM buffer of
    rows of 512 residues (the [K][2][L][N] order), each row holding the C learners' slices
    side by side, every residue of tower t packed to U_t bits (bitlength(q_t) when that is 1
    mod 4, else rounded up to a multiple of 4; 60 / 53 / 52 / 53 at 2^15 / L4: 218 of 256 bits
    per coefficient).  put()
    packs and validates each learner's batch once per round; wavg() then reads one
    contiguous C-slice region per row and writes the [K][2][L][N] uint64 aggregate."""

    # layout="auto": arenas of at most this many 512-residue rows per learner (K * 2 * L * N / 512)
    # take the uint64 layout.  A packed launch is one wave per row over all C learners; a grid of
    # a few thousand rows (cfg2: 2,048 rows = 2 waves per SIMD) cannot hide its ramp and tail, and
    # wavg_kernel's 4x as many shorter waves over uint64 batches run it 7% faster (cfg2: 23.3 vs
    # 25.0 us per launch, profiles/r04f/wavg_small_ab.txt); at 4,096 rows (16 x 8 cts) the two
    # are level (46.8 vs 46.7 us), and from cfg5's 79,872 rows on the packed bytes win.
    AUTO_U64_ROWS = 4096
    # uint64 layout: words of padding after each learner's slot.  A slot of K ciphertexts at
    # 2^15 / L4 is K * 2^21 bytes: unpadded, a thread's C loads sit a power of two apart and the
    # launch runs 15% slower (26.9 vs 23.3 us at cfg2; 4 KiB beat 256 B, 32 KiB and 512 KiB,
    # profiles/r04f/wavg_small_ab.txt)
    SLOT_PAD_WORDS = 512

    def __init__(self, ckks, num_learners: int, K: int, device=None, layout: str = "packed",
                 slot_pad: int | None = None):
        torch = _torch()
        self.ckks, self.C, self.K = ckks, int(num_learners), int(K)
        inf = ckks.info()
        self.L, self.N = inf["num_towers"], inf["ring_dim"]
        if device is None:
            device = "cuda:%d" % inf["device"]
        if layout == "auto":
            layout = "uint64" if self.K * 2 * self.L * (self.N // 512) <= self.AUTO_U64_ROWS else "packed"
        if layout not in ("packed", "uint64"):
            raise ValueError("layout must be 'packed', 'uint64' or 'auto'")
        self.layout = layout
        lib = _lib.load()
        # the packed layout is sized by the context's moduli: an arena belongs to this parameter
        # generation (loadCryptoParams / genCryptoContextAndKeyGen start a new one)
        self._gen = getattr(ckks, "_params_gen", 0)
        if layout == "uint64":
            # C learner batches [K][2][L][N] one after the other, aggregated by wavg_kernel
            self.ct_words = 2 * self.L * self.N
            pad = self.SLOT_PAD_WORDS if slot_pad is None else int(slot_pad)
            self._slot_stride = self.K * self.ct_words + pad  # words
            self.buf = torch.empty(self.C * self._slot_stride, dtype=torch.int64, device=device)
            self.data_bytes = self.C * self.K * self.ct_words * 8
            self._refused = set()
            # per first ciphertext k0: the C slots' pointers, built once.  A cfg2 launch takes
            # ~25 us; sixteen tensor slices and checks per call took longer than that on the host
            # and left the GPU waiting (bench.py cfg2: 43 us per step, profiles/r04d)
            self._slot_ptrs = {}
            return
        self.ct_words = lib.shelfi_arena_words(ckks._ctx, self.C, 1)  # packed words per ciphertext
        words = lib.shelfi_arena_words(ckks._ctx, self.C, self.K)
        self.buf = torch.empty(words, dtype=torch.int64, device=device)
        self.data_bytes = words * 8

    def _slot(self, learner: int):
        """uint64 layout: learner `learner`'s [K][2][L][N] batch in the arena (a writable view; only
        put() writes through it, so every placed residue is validated)."""
        if self.layout != "uint64":
            raise ValueError("learner slots are the uint64 layout's; the packed layout interleaves learners")
        o = int(learner) * self._slot_stride
        return self.buf[o:o + self.K * self.ct_words].view(self.K, 2, self.L, self.N)

    def slot(self, learner: int):
        """uint64 layout: a copy of learner `learner`'s placed [K][2][L][N] batch.  A copy, not a
        view: writes into the arena go through put(), which checks every residue < q_t (the
        aggregation's carry-free limb sums assume canonical residues)."""
        return self._slot(learner).clone()

    def release(self):
        """Drop this arena's refusal marks in the context and free its memory."""
        buf = getattr(self, "buf", None)
        if buf is None:
            return
        ctx = getattr(self.ckks, "_ctx", None)
        if self.layout == "packed" and ctx is not None and getattr(ctx, "value", None):
            _lib.load().shelfi_dev_arena_release(ctx, C.c_void_p(buf.data_ptr()), buf.numel())
        self.buf = None
        self._out = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def _check_gen(self):
        if getattr(self, "buf", None) is None:
            raise ValueError("the arena was released")
        if getattr(self.ckks, "_params_gen", 0) != self._gen:
            raise ValueError("the context's parameters or keys were reloaded since this arena was "
                             "made: its packed layout no longer matches; make a new Arena")

    def put(self, learner: int, ct):
        """Place learner `learner`'s batch: a [K][2][L][N] CUDA tensor, or its upload as it
        came over the wire (a library blob or a PALISADE archive, bytes-like).  An upload's
        header is checked against the context (parameters, key, length, K) before any copy;
        every put then checks that each placed residue is < q_t, and a refused slot keeps
        wavg() failing until a valid put replaces it (shelfi_dev_arena_put[_blob])."""
        self._check_gen()
        if self.layout == "uint64":
            self._put_u64(int(learner), ct)
            return
        if isinstance(ct, (bytes, bytearray, memoryview)):
            import numpy as np

            host = np.frombuffer(ct, dtype=np.uint8)
            check(_lib.load().shelfi_dev_arena_put_blob(self.ckks._ctx, C.c_void_p(host.ctypes.data), host.size,
                                                        self.K, int(learner), self.C,
                                                        C.c_void_p(self.buf.data_ptr()),
                                                        C.c_void_p(_stream_ptr(self.buf))), "arena_put")
            return
        _check_ct(ct, self.ckks, self.K)
        if ct.device != self.buf.device:
            raise ValueError("the batch must live on the arena's device")
        check(_lib.load().shelfi_dev_arena_put(self.ckks._ctx, C.c_void_p(ct.data_ptr()), 0, self.K,
                                               int(learner), self.C, C.c_void_p(self.buf.data_ptr()),
                                               C.c_void_p(_stream_ptr(ct))), "arena_put")

    def _put_u64(self, learner: int, ct):
        """uint64 layout: the batch lands in its slot and is checked (residues < q_t); an upload is
        validated exactly as the packed layout's (header against the context, then residues) by
        placing it in a one-learner packed arena and summing that with unit weight into the slot."""
        if not (0 <= learner < self.C):
            raise ValueError("learner index outside the arena")
        self._refused.add(learner)  # until this put has landed and passed its checks
        if isinstance(ct, (bytes, bytearray, memoryview)):
            tmp = Arena(self.ckks, 1, self.K, device=self.buf.device, layout="packed")
            tmp.put(0, ct)
            sum_packed(self.ckks, tmp.buf, 1, self.K, tmp.ct_words * self.K, out=self._slot(learner))
            tmp.release()
        else:
            _check_ct(ct, self.ckks, self.K)
            if ct.device != self.buf.device:
                raise ValueError("the batch must live on the arena's device")
            dst = self._slot(learner)
            dst.copy_(ct)
            check(_lib.load().shelfi_dev_check_residues(self.ckks._ctx, C.c_void_p(dst.data_ptr()),
                                                        self.K, C.c_void_p(_stream_ptr(self.buf))),
                  "arena_put: learner %d" % learner)
        self._refused.discard(learner)

    def wavg(self, weights: Sequence[float], out=None, k0: int = 0, k1: int | None = None):
        """Aggregate ciphertexts [k0, k1) of every learner into out[:k1-k0]."""
        torch = _torch()
        self._check_gen()
        if len(weights) != self.C:
            raise ValueError("need one weight per learner")
        k1 = self.K if k1 is None else int(k1)
        if not (0 <= k0 <= k1 <= self.K):
            raise ValueError("bad ciphertext range")
        Kr = k1 - k0
        if out is None:
            out = torch.empty((Kr, 2, self.L, self.N), dtype=torch.int64, device=self.buf.device)
        _check_ct(out, self.ckks, Kr)
        if self.layout == "uint64":
            if self._refused:
                raise _lib.ShelfiError(_lib.SHELFI_ERR_STATE, "dev_wavg_arena: the arena holds a refused upload "
                                       "for learner %d; put a valid batch first" % min(self._refused))
            ptrs = self._slot_ptrs.get(k0)
            if ptrs is None:
                base, slot = self.buf.data_ptr() + k0 * self.ct_words * 8, self._slot_stride * 8
                ptrs = self._slot_ptrs[k0] = (C.c_void_p * self.C)(*[base + c * slot for c in range(self.C)])
            w = (C.c_float * self.C)(*[float(x) for x in weights])
            check(_lib.load().shelfi_dev_wavg(self.ckks._ctx, ptrs, w, self.C, Kr, C.c_void_p(out.data_ptr()),
                                              C.c_void_p(_stream_ptr(out))), "dev_wavg_arena")
            return out
        w = (C.c_float * self.C)(*[float(x) for x in weights])
        # ciphertexts [k0, k1) of an arena are themselves an arena of k1-k0 ciphertexts
        base = self.buf.data_ptr() + k0 * self.ct_words * 8
        check(_lib.load().shelfi_dev_wavg_arena(self.ckks._ctx, C.c_void_p(base), w, self.C, Kr,
                                                C.c_void_p(out.data_ptr()),
                                                C.c_void_p(_stream_ptr(out))), "dev_wavg_arena")
        return out


    def wavg_packed(self, weights: Sequence[float], out=None, k0: int = 0, k1: int | None = None):
        """wavg() with the aggregate written packed (the slice format with C = 1; a flat int64
        tensor of packed_words(k1 - k0) words): the packed share exchange's send form."""
        torch = _torch()
        self._check_gen()
        if self.layout != "packed":
            raise ValueError("a packed aggregate comes from the packed layout (Arena(..., layout='packed'))")
        if len(weights) != self.C:
            raise ValueError("need one weight per learner")
        k1 = self.K if k1 is None else int(k1)
        if not (0 <= k0 <= k1 <= self.K):
            raise ValueError("bad ciphertext range")
        need = packed_words(self.ckks, k1 - k0)
        if out is None:
            out = torch.empty(need, dtype=torch.int64, device=self.buf.device)
        if not out.is_cuda or out.dtype != torch.int64 or out.numel() < need or not out.is_contiguous():
            raise ValueError("out must be a contiguous int64 CUDA tensor of >= %d words" % need)
        w = (C.c_float * self.C)(*[float(x) for x in weights])
        base = self.buf.data_ptr() + k0 * self.ct_words * 8
        check(_lib.load().shelfi_dev_wavg_arena_packed(self.ckks._ctx, C.c_void_p(base), w, self.C, k1 - k0,
                                                       C.c_void_p(out.data_ptr()),
                                                       C.c_void_p(_stream_ptr(out))), "dev_wavg_arena_packed")
        return out

    def output(self, candidates: int = 8, include=()):
        """The arena's own aggregate buffer ([K][2][L][N] int64, reused: ``ar.wavg(w, out=ar.output())``
        overwrites it), placed for this arena when first asked for.  A packed launch runs up to ~14%
        slower for some (arena, output) pairs of physical HBM regions -- a property of the pair, not of
        either buffer (tools/placement_probe2.py) -- so the first call times one
        launch into each of `candidates` fresh buffers (and the tensors in `include`) and keeps the
        fastest (place_output); later calls return the same buffer.  The uint64 layout, or an arena with
        a refused upload, takes a plain buffer.  output_placement holds the candidates' launch times."""
        torch = _torch()
        self._check_gen()
        if getattr(self, "_out", None) is None:
            ms = []
            out = None
            if self.layout == "packed" and candidates + len(include) > 0:
                try:
                    out, ms = self.place_output([1.0 / self.C] * self.C, candidates=candidates, launches=2,
                                                include=include)
                except _lib.ShelfiError:  # a refused upload: no launch to time
                    out, ms = None, []
            if out is None:
                out = include[0] if include else torch.empty((self.K, 2, self.L, self.N), dtype=torch.int64,
                                                             device=self.buf.device)
            self._out, self.output_placement = out, ms
        return self._out

    def place_output(self, weights: Sequence[float], candidates: int = 8, launches: int = 2, include=()):
        """A [K][2][L][N] output buffer placed well for this arena.  The launch time
        depends on where the output lands in physical HBM relative to the arena (up to
        12%, reproducible per buffer pair), so `candidates` buffers are
        allocated side by side, timed (shelfi_dev_wavg_arena_pick_output) and all but the
        fastest released; buffers in `include` (already allocated [K][2][L][N] tensors) are
        candidates too, ahead of the new ones.  Returns (buffer, per-candidate ms)."""
        torch = _torch()
        self._check_gen()
        if self.layout != "packed":  # separate batches: no placement search
            out = include[0] if include else torch.empty((self.K, 2, self.L, self.N), dtype=torch.int64,
                                                         device=self.buf.device)
            self.wavg(weights, out=out)
            return out, []
        cands = list(include)
        for c in cands:
            _check_ct(c, self.ckks, self.K)
        cands += [torch.empty((self.K, 2, self.L, self.N), dtype=torch.int64, device=self.buf.device)
                  for _ in range(max(1 if not cands else 0, int(candidates)))]
        ptrs = (C.c_void_p * len(cands))(*[t.data_ptr() for t in cands])
        w = (C.c_float * self.C)(*[float(x) for x in weights])
        best = C.c_size_t()
        ms = (C.c_float * len(cands))()
        check(_lib.load().shelfi_dev_wavg_arena_pick_output(
            self.ckks._ctx, C.c_void_p(self.buf.data_ptr()), w, self.C, self.K, ptrs, len(cands),
            int(launches), C.byref(best), ms, C.c_void_p(_stream_ptr(self.buf))), "arena_pick_output")
        out = cands[best.value]
        del cands
        return out, [round(float(x), 4) for x in ms]


def packed_words(ckks, K: int) -> int:
    """64-bit words of K ciphertexts in the packed C = 1 slice format (the packed wire / exchange)."""
    return int(_lib.load().shelfi_arena_words(ckks._ctx, 1, int(K)))


def sum_packed(ckks, stacked, G: int, K: int, stride: int, out=None):
    """sum_g x_g mod q_t of G packed (C = 1) batches of K ciphertexts stacked `stride` words apart
    in the int64 tensor `stacked` -> [K][2][L][N] (shelfi_dev_sum_packed)."""
    torch = _torch()
    if not stacked.is_cuda or stacked.dtype != torch.int64 or not stacked.is_contiguous():
        raise ValueError("stacked must be a contiguous int64 CUDA tensor")
    if K and (stride < packed_words(ckks, K) or stacked.numel() < (G - 1) * stride + packed_words(ckks, K)):
        raise ValueError("stacked is smaller than G batches of K ciphertexts at that stride")
    if out is None:
        out = empty_ct(ckks, K, device=stacked.device)
    _check_ct(out, ckks, K)
    check(_lib.load().shelfi_dev_sum_packed(ckks._ctx, C.c_void_p(stacked.data_ptr()), int(G), int(K), int(stride),
                                            C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(out))),
          "dev_sum_packed")
    return out


def modq(ckks, buf):
    """Fold a collective's uint64 sum of <= 15 partial sums back into [0, q_t)."""
    _check_ct(buf, ckks)
    check(_lib.load().shelfi_dev_modq(ckks._ctx, C.c_void_p(buf.data_ptr()), buf.shape[0],
                                      C.c_void_p(_stream_ptr(buf))), "dev_modq")
    return buf


def encrypt(ckks, x, out=None):
    """encode + encrypt a float64 CUDA vector into ceil(n / V) ciphertexts, V = info()["values_per_ct"]: batch,
    or 2 * batch under complex slot packing (CKKS.set_slot_packing; x is then the float64 view of a complex128
    vector)."""
    torch = _torch()
    if not x.is_cuda or x.dtype != torch.float64:
        raise ValueError("x must be a float64 CUDA tensor")
    x = x.contiguous().view(-1)
    B = ckks.info()["values_per_ct"]
    K = (x.numel() + B - 1) // B
    if out is None:
        out = empty_ct(ckks, K, x.device)
    _check_ct(out, ckks, K)
    check(_lib.load().shelfi_dev_encrypt(ckks._ctx, C.c_void_p(x.data_ptr()), x.numel(),
                                         C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(x))),
          "dev_encrypt")
    return out


def decrypt(ckks, ct, n: int, scale: float, out=None):
    """decrypt + decode K ciphertexts of scaling factor `scale` into n float64 values
    (any number of towers <= L: ciphertexts after rescale() decrypt at their level)."""
    torch = _torch()
    _check_ct(ct, ckks, any_level=True)
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=ct.device)
    check(_lib.load().shelfi_dev_decrypt_level(ckks._ctx, C.c_void_p(ct.data_ptr()), ct.shape[0],
                                               int(ct.shape[2]), float(scale), int(n),
                                               C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(ct))),
          "dev_decrypt")
    return out


def decrypt_sum(ckks, ct, terms: int, n: int, scale: float, out=None):
    """decrypt a multi-GPU combine's unfolded share: every residue is a uint64 sum of `terms`
    (<= 16) canonical residues (Comm.combine_arena(fold=False)); the mod-q fold happens in
    decrypt's first pass (shelfi_dev_decrypt_sum)."""
    torch = _torch()
    _check_ct(ct, ckks)
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=ct.device)
    check(_lib.load().shelfi_dev_decrypt_sum(ckks._ctx, C.c_void_p(ct.data_ptr()), ct.shape[0], int(terms),
                                             float(scale), int(n), C.c_void_p(out.data_ptr()),
                                             C.c_void_p(_stream_ptr(ct))), "dev_decrypt_sum")
    return out


def partial_decrypt(ckks, ct, lead: bool, out=None):
    """This party's partial decryption of K ciphertexts (any number of towers <= L) with the context's
    key share and smudging noise (CKKS.set_threshold_noise): [K][2][l][N] -> [K][l][N], lead: c0 + c1 s
    + e (MultipartyDecryptLead), else c1 s + e (MultipartyDecryptMain)."""
    torch = _torch()
    _check_ct(ct, ckks, any_level=True)
    K, _, l, N = ct.shape
    if out is None:
        out = torch.empty((K, l, N), dtype=ct.dtype, device=ct.device)
    if (not out.is_cuda or not out.is_contiguous() or out.element_size() != 8 or tuple(out.shape) != (K, l, N)
            or out.device != ct.device):
        raise ValueError("out must be a contiguous [K][l][N] 64-bit tensor on ct's device")
    check(_lib.load().shelfi_dev_partial_decrypt(ckks._ctx, C.c_void_p(ct.data_ptr()), K, int(l), 1 if lead else 0,
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(ct))),
          "dev_partial_decrypt")
    return out


def fuse_decrypt(ckks, partials: Sequence, n: int, scale: float, out=None):
    """MultipartyDecryptFusion of 1..16 partial decryptions [K][l][N] (device tensors of one shape on one
    device) into n float64 values; needs no keys.  The partials are summed while decrypt's first pass
    loads them; the rest is decrypt()'s chain."""
    torch = _torch()
    partials = list(partials)
    L, N = _ln(ckks)
    if partials:
        p0 = partials[0]
        for p in partials:
            if (not p.is_cuda or not p.is_contiguous() or p.element_size() != 8 or p.dim() != 3
                    or p.shape != p0.shape or p.device != p0.device or p.shape[2] != N):
                raise ValueError("partials must be contiguous 64-bit CUDA tensors of one shape [K][l][N]")
        K, towers, dev = int(p0.shape[0]), int(p0.shape[1]), p0.device
    else:
        K, towers, dev = 0, L, "cuda:%d" % ckks.info()["device"]
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=dev)
    ptrs = (C.c_void_p * max(1, len(partials)))(*[p.data_ptr() for p in partials])
    stream = _stream_ptr(partials[0]) if partials else 0
    check(_lib.load().shelfi_dev_fuse_decrypt(ckks._ctx, ptrs, len(partials), K, towers, float(scale), int(n),
                                              C.c_void_p(out.data_ptr()), C.c_void_p(stream)), "dev_fuse_decrypt")
    return out


def mult(ckks, a, b, out=None):
    """cc->EvalMult(a, b) for K ciphertext pairs of the same level: tensor product +
    HYBRID relinearization (needs ckks.evalMultKeyGen()).  Scale: scale_a * scale_b."""
    torch = _torch()
    _check_ct(a, ckks, any_level=True)
    _check_ct(b, ckks, a.shape[0], any_level=True)
    if a.shape != b.shape:
        raise ValueError("EvalMult operands must have the same shape (same level)")
    if b.device != a.device:
        raise ValueError("EvalMult operands must live on the same device")
    if out is None:
        out = torch.empty_like(a)
    _check_ct(out, ckks, a.shape[0], any_level=True)
    if out.shape != a.shape or out.device != a.device:
        raise ValueError("out must be a contiguous tensor shaped like a, on a's device")
    check(_lib.load().shelfi_dev_mult(ckks._ctx, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), a.shape[0],
                                      int(a.shape[2]), C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(a))),
          "dev_mult")
    return out


def dot(ckks, a, b, out=None):
    """cc->EvalInnerProduct's body over K ciphertext pairs of the same level: sum_k a_k (x) b_k as one
    three-component tensor, relinearized once (needs ckks.evalMultKeyGen()) -> one ciphertext
    [1][2][l][N] whose slots hold sum_k x_k[i] y_k[i].  It decrypts to what the sum of K mult()s decrypts
    to, with one key switch instead of K.  a is b (or the same storage) takes the squared path, reading
    each ciphertext once.  out must overlap neither input.  Scale: scale_a * scale_b."""
    torch = _torch()
    _check_ct(a, ckks, any_level=True)
    _check_ct(b, ckks, a.shape[0], any_level=True)
    if a.shape != b.shape:
        raise ValueError("EvalInnerProduct operands must have the same shape (same level)")
    if b.device != a.device:
        raise ValueError("EvalInnerProduct operands must live on the same device")
    K, _, l, N = a.shape
    if K == 0:  # (an empty tensor has no storage to hand the library, which refuses K = 0 by name)
        raise ValueError("EvalInnerProduct needs at least one ciphertext pair")
    if out is None:
        out = torch.empty((1, 2, l, N), dtype=a.dtype, device=a.device)
    _check_ct(out, ckks, 1, any_level=True)
    if tuple(out.shape) != (1, 2, l, N) or out.device != a.device:
        raise ValueError("out must be a contiguous [1][2][l][N] 64-bit tensor on a's device")
    check(_lib.load().shelfi_dev_dot(ckks._ctx, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), K, int(l),
                                     C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(a))), "dev_dot")
    return out


GRAM_MAX_BATCHES = 32  # shelfi_dev_gram: the batches' base pointers travel in the kernel arguments


def gram_pairs(C: int):
    """The pairs (i, j), i <= j, in the order device.gram writes them: the upper triangle, row-major;
    (i, j) sits at i C - i (i - 1) / 2 + (j - i)."""
    return [(i, j) for i in range(int(C)) for j in range(i, int(C))]


def gram(ckks, batches, out=None):
    """The Gram matrix of C batches of K ciphertexts at one level (needs ckks.evalMultKeyGen()): a batch
    [P][2][l][N] of P = C (C + 1) / 2 ciphertexts, the one at gram_pairs(C).index((i, j)) being exactly
    dot(ckks, batches[i], batches[j]), bit for bit -- its slots hold sum_k x_ik[s] x_jk[s] -- at one pass over
    the inputs per tile of 2 x 2 batches and one batched key switch.  batches: a sequence of 1..32 tensors
    [K][2][l][N] (the same tensor may appear twice), or one stacked [C][K][2][l][N] tensor.  out must overlap
    no input.  Scale: scale^2.  rescale, eval_sum, add, sub, decrypt and partial_decrypt take the result as
    any batch of P ciphertexts."""
    torch = _torch()
    if hasattr(batches, "dim"):
        if batches.dim() != 5 or not batches.is_contiguous():
            raise ValueError("a stacked Gram operand must be a contiguous [C][K][2][l][N] tensor")
        batches = [batches[i] for i in range(batches.shape[0])]
    batches = list(batches)
    n = len(batches)
    if not 1 <= n <= GRAM_MAX_BATCHES:
        raise ValueError("Gram needs 1..%d batches" % GRAM_MAX_BATCHES)
    a = batches[0]
    _check_ct(a, ckks, any_level=True)
    for b in batches[1:]:
        _check_ct(b, ckks, a.shape[0], any_level=True)
        if b.shape != a.shape:
            raise ValueError("Gram operands must have the same shape (same level)")
        if b.device != a.device:
            raise ValueError("Gram operands must live on the same device")
    K, _, l, N = a.shape
    if K == 0:  # (an empty tensor has no storage to hand the library, which refuses K = 0 by name)
        raise ValueError("Gram needs at least one ciphertext a batch")
    P = n * (n + 1) // 2
    if out is None:
        out = torch.empty((P, 2, l, N), dtype=a.dtype, device=a.device)
    _check_ct(out, ckks, P, any_level=True)
    if tuple(out.shape) != (P, 2, l, N) or out.device != a.device:
        raise ValueError("out must be a contiguous [C (C + 1) / 2][2][l][N] 64-bit tensor on the batches' device")
    ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in batches])
    check(_lib.load().shelfi_dev_gram(ckks._ctx, ptrs, n, K, int(l), C.c_void_p(out.data_ptr()),
                                      C.c_void_p(_stream_ptr(a))), "dev_gram")
    return out


WSUM_MAX_LEARNERS = 32  # shelfi_dev_wsum_ct: as GRAM_MAX_BATCHES, for the updates and for the weights


def _unstack(t, what):
    if hasattr(t, "dim"):
        if t.dim() != 5 or not t.is_contiguous():
            raise ValueError("a stacked %s operand must be a contiguous [C][K][2][l][N] tensor" % what)
        return [t[i] for i in range(t.shape[0])]
    return list(t)


def wsum_ct(ckks, batches, weights, out=None):
    """EvalLinearWSum with ENCRYPTED weights (needs ckks.evalMultKeyGen()): out[k] = sum_c weights[c] * batches[c][k]
    over C learners, with one key switch per output ciphertext instead of one per product.  batches: a sequence of
    1..32 update tensors [K][2][lu][N], or one stacked [C][K][2][lu][N] tensor; weights: as many tensors
    [Kw][2][l][N], or one stacked tensor, with Kw = 1 (one weight ciphertext for a learner's whole update) or Kw = K
    (one per update ciphertext).  The result [K][2][l][N] is, bit for bit, dot() of the stacked weights against the
    stacked k-th update ciphertexts, and at C = 1 mult(weight, update).  out must overlap no input.
    Scale: scale_w * scale_u, depth 2: rescale() it as a mult() result, then add / decrypt / partial_decrypt.
    Level rule: lu >= l.  Weights that come out of a computation sit lower than fresh updates; the first l towers of
    every update polynomial are read in place (dropping towers of an RNS ciphertext is only a stride), and the result
    sits at the weights' level l."""
    torch = _torch()
    batches, weights = _unstack(batches, "update"), _unstack(weights, "weight")
    n = len(batches)
    if not 1 <= n <= WSUM_MAX_LEARNERS:
        raise ValueError("EvalLinearWSum needs 1..%d learners" % WSUM_MAX_LEARNERS)
    if len(weights) != n:
        raise ValueError("EvalLinearWSum needs one weight batch per update batch")
    u, w = batches[0], weights[0]
    _check_ct(u, ckks, any_level=True)
    _check_ct(w, ckks, any_level=True)
    for b in batches[1:]:
        _check_ct(b, ckks, any_level=True)
        if b.shape != u.shape:
            raise ValueError("EvalLinearWSum updates must have the same shape (same level)")
    for b in weights[1:]:
        _check_ct(b, ckks, any_level=True)
        if b.shape != w.shape:
            raise ValueError("EvalLinearWSum weights must have the same shape (same level)")
    if any(b.device != u.device for b in batches + weights):
        raise ValueError("EvalLinearWSum operands must live on the same device")
    K, _, lu, N = u.shape
    Kw, _, l, _ = w.shape
    if K == 0:  # (an empty tensor has no storage to hand the library, which refuses K = 0 by name)
        raise ValueError("EvalLinearWSum needs at least one update ciphertext a learner")
    if Kw not in (1, K):
        raise ValueError("EvalLinearWSum weights are [1 or K][2][l][N]: one ciphertext for all updates, or one each")
    if l > lu:
        raise ValueError("EvalLinearWSum updates must sit at the weights' level or above")
    if out is None:
        out = torch.empty((K, 2, l, N), dtype=u.dtype, device=u.device)
    _check_ct(out, ckks, K, any_level=True)
    if tuple(out.shape) != (K, 2, l, N) or out.device != u.device:
        raise ValueError("out must be a contiguous [K][2][l][N] 64-bit tensor at the weights' level on the operands' device")
    up = (C.c_void_p * n)(*[b.data_ptr() for b in batches])
    wp = (C.c_void_p * n)(*[b.data_ptr() for b in weights])
    check(_lib.load().shelfi_dev_wsum_ct(ckks._ctx, up, n, K, int(lu), wp, Kw, int(l), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(_stream_ptr(u))), "dev_wsum_ct")
    return out


def _poly_plan(ckks, coeffs, towers, scale, combine_scale=None):
    from . import poly

    inf = ckks.info()
    return poly.plan(inf["moduli"], inf["scale_bits"], coeffs, towers, scale, combine_scale)


def _poly_powers(ckks, x, pl):
    """{n: (P_n, scale)} along the plan's schedule: a product is wsum_ct at C = 1 -- the operand stored higher as
    the update, read in place over the lower one's towers -- and one rescale."""
    have = {}
    for p in pl["powers"]:
        if p["n"] == 1:
            have[1] = (x, p["scale"])
            continue
        a, b = have[p["a"]][0], have[p["b"]][0]
        hi, lo = (a, b) if a.shape[2] >= b.shape[2] else (b, a)
        have[p["n"]] = (rescale(ckks, wsum_ct(ckks, [hi], [lo])), p["scale"])
    return have


def poly_powers(ckks, x, scale: float, degree: int):
    """The powers of x [K][2][l][N] (at `scale`) that eval_poly of a degree-`degree` polynomial needs (needs
    ckks.evalMultKeyGen()): {n: (P_n, scale_n)} for n = 1, 2, 3 as far as the degree reaches and n = 4, 8, 12, ..
    below it, along shelfi_poly_plan's schedule (P_2 = P_1 P_1, P_3 = P_2 P_1, P_4 = P_2 P_2, P_{4g} = P_{4h}
    P_{4(g-h)}).  Every product is one key switch a ciphertext and one rescale; P_n sits ceil(log2 n) towers below
    x and its scale is the exact one.  The plan is made for the whole evaluation: an input with too few towers for the
    combine's 1 or 2 rescales is refused here too, though the powers alone would fit."""
    _check_ct(x, ckks, any_level=True)
    if x.shape[0] == 0:
        raise ValueError("EvalPoly needs at least one ciphertext")
    if not 1 <= int(degree) <= 31:
        raise ValueError("EvalPoly takes degrees 1..31")
    return _poly_powers(ckks, x, _poly_plan(ckks, [0.0] * (int(degree) + 1), int(x.shape[2]), scale))


def poly_combine(ckks, babies, giants, table, towers: int, out=None):
    """shelfi_dev_poly_combine: babies = [P_1, ..] (1..3 batches), giants = [P_4, P_8, ..] (0..7), each
    [K][2][its towers][N] with its towers >= `towers`, read in place; table: the plan's uint64 residues
    [len(giants) + 1][4][towers].  out [K][2][towers][N] = (d0, d1) + KeySwitch(d2) of the summed giant-step
    products (include/shelfi.h), at the plan's combine scale; out must overlap no operand.  Without giants no
    evaluation key is needed."""
    import numpy as np

    torch = _torch()
    babies, giants = list(babies), list(giants)
    if not 1 <= len(babies) <= 3 or len(giants) > 7:
        raise ValueError("EvalPoly's combine takes 1..3 baby-step and 0..7 giant-step powers")
    ops = babies + giants
    x = ops[0]
    for t in ops:
        _check_ct(t, ckks, x.shape[0] if t is not x else None, any_level=True)
        if t.device != x.device:
            raise ValueError("EvalPoly operands must live on the same device")
    K, _, _, N = x.shape
    towers = int(towers)
    if K == 0:
        raise ValueError("EvalPoly needs at least one ciphertext")
    if towers < 1 or any(t.shape[2] < towers for t in ops):
        raise ValueError("EvalPoly: every power must sit at the combine level or above")
    tab = np.ascontiguousarray(table, dtype=np.uint64)
    if tab.shape != (len(giants) + 1, 4, towers):
        raise ValueError("EvalPoly's constants are [giants + 1][4][towers] uint64 residues")
    if out is None:
        out = torch.empty((K, 2, towers, N), dtype=x.dtype, device=x.device)
    _check_ct(out, ckks, K, any_level=True)
    if tuple(out.shape) != (K, 2, towers, N) or out.device != x.device:
        raise ValueError("out must be a contiguous [K][2][towers][N] 64-bit tensor on the operands' device")
    bp = (C.c_void_p * 3)(*[t.data_ptr() for t in babies])
    bt = (C.c_uint32 * 3)(*[int(t.shape[2]) for t in babies])
    gp = (C.c_void_p * 7)(*[t.data_ptr() for t in giants])
    gt = (C.c_uint32 * 7)(*[int(t.shape[2]) for t in giants])
    check(_lib.load().shelfi_dev_poly_combine(ckks._ctx, bp, bt, len(babies), gp, gt, len(giants),
                                              tab.ctypes.data_as(_lib.u64p), K, towers, C.c_void_p(out.data_ptr()),
                                              C.c_void_p(_stream_ptr(x))), "dev_poly_combine")
    return out


def eval_poly(ckks, x, coeffs, scale: float, combine_scale=None):
    """cc->EvalPoly: p(x) = sum_i coeffs[i] x^i in every slot of the K ciphertexts x [K][2][l][N] at `scale`,
    degree 1..31 (needs ckks.evalMultKeyGen() from degree 2 on).  Returns (ct, scale_out).

    Paterson-Stockmeyer with four baby steps: the powers x, x^2, x^3, x^4, x^8, x^12, .. (poly_powers: one key switch
    and one rescale each), then ONE combine pass that sums every giant-step product x^{4g} q_g(x) as one tensor and
    relinearizes it once per ciphertext (poly_combine), then 1 (degree <= 3) or 2 rescales.  Key switches per
    ciphertext: 2 at degree 3, 4 at 7, 6 at 15 -- against degree - 1 for a term-by-term composition.  The constants
    are encoded at scales that absorb each power's exact scale (SHELFI_FHE.poly.plan), so the differing rescales of
    the powers cost no precision; combine_scale overrides the scale the terms are summed at (default 2^{2p}, or
    2^{3p} above degree 3, p the context's scaling bits).
    Levels: the result sits ceil(log2(highest power)) + rescales towers below x -- 3 at degree 3, 4 at 7, 6 at 15,
    7 from 20 on; too few towers and constants too large for the combine level are ValueErrors.  Fit coefficients
    on a normalised input (SHELFI_FHE.poly.fit)."""
    _check_ct(x, ckks, any_level=True)
    if x.shape[0] == 0:
        raise ValueError("EvalPoly needs at least one ciphertext")
    pl = _poly_plan(ckks, coeffs, int(x.shape[2]), scale, combine_scale)
    have = _poly_powers(ckks, x, pl)
    babies = [have[j][0] for j in range(1, pl["babies"] + 1)]
    giants = [have[4 * g][0] for g in range(1, pl["giants"])]
    out = poly_combine(ckks, babies, giants, pl["table"], pl["combine_towers"])
    for _ in range(pl["rescales"]):
        out = rescale(ckks, out)
    return out, pl["result_scale"]


def gram_sq_distances(ckks, G, n: int, out=None):
    """Krum's input from gram()'s result G [P][2][l][N] over n batches: the n (n - 1) / 2 ciphertexts
    G_ii + G_jj - 2 G_ij of ||u_i - u_j||^2 for i < j, in gram_pairs(n)'s order without the diagonal.  Index
    gathers and the existing add / sub: no key, no new level, G's scale."""
    torch = _torch()
    n = int(n)
    _check_ct(G, ckks, n * (n + 1) // 2, any_level=True)
    if n < 2:
        raise ValueError("squared distances need at least two batches")
    pairs = gram_pairs(n)
    at = {p: k for k, p in enumerate(pairs)}
    off = [p for p in pairs if p[0] != p[1]]

    def take(idx):
        return G.index_select(0, torch.tensor(idx, dtype=torch.int64, device=G.device))

    ij = take([at[p] for p in off])
    out = add(ckks, take([at[(i, i)] for i, _ in off]), take([at[(j, j)] for _, j in off]), out=out)
    sub(ckks, out, ij, out=out)
    return sub(ckks, out, ij, out=out)


def rescale(ckks, ct, out=None):
    """cc->ModReduce(ct): drop the last tower, dividing by it with rounding
    ([K][2][l][N] -> [K][2][l-1][N]); scale / q_{l-1}."""
    torch = _torch()
    _check_ct(ct, ckks, any_level=True)
    K, _, l, N = ct.shape
    if l < 2:
        raise ValueError("ModReduce needs at least 2 towers")
    if out is None:
        out = torch.empty((K, 2, l - 1, N), dtype=ct.dtype, device=ct.device)
    _check_ct(out, ckks, K, any_level=True)
    if tuple(out.shape) != (K, 2, l - 1, N) or out.device != ct.device:
        raise ValueError("out must be a contiguous [K][2][l-1][N] 64-bit tensor on ct's device")
    check(_lib.load().shelfi_dev_rescale(ckks._ctx, C.c_void_p(ct.data_ptr()), K, int(l),
                                         C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(ct))), "dev_rescale")
    return out


def _like(ckks, ct, out):
    """out (or a new tensor) shaped like the ciphertext batch ct, on its device."""
    if out is None:
        return _torch().empty_like(ct)
    _check_ct(out, ckks, ct.shape[0], any_level=True)
    if out.shape != ct.shape or out.device != ct.device:
        raise ValueError("out must be a contiguous tensor shaped like the input, on its device")
    return out


def rotate(ckks, ct, r: int, out=None):
    """cc->EvalAtIndex(ct, r) for K ciphertexts of any level: slot i of the result holds slot
    (i + r) mod batch of the input (r > 0 rotates left).  Needs ckks.rotationKeyGen([r]) (or any index
    with the same Galois element); r = 0 is a copy.  out must not overlap ct.  Scale unchanged."""
    _check_ct(ct, ckks, any_level=True)
    out = _like(ckks, ct, out)
    check(_lib.load().shelfi_dev_rotate(ckks._ctx, C.c_void_p(ct.data_ptr()), ct.shape[0], int(ct.shape[2]), int(r),
                                        C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(ct))), "dev_rotate")
    return out


ROTATE_MANY_MAX = 64  # shelfi_dev_rotate_many: the keys a context holds


def rotate_many(ckks, ct, rs, out=None):
    """The rotations of K ciphertexts by every index of rs from ONE digit decomposition of their c1 (hoisting:
    PALISADE's EvalFastRotationPrecompute / EvalFastRotation): a tensor [R][K][2][l][N] whose entry r is an
    ordinary batch holding rotate(ct, rs[r])'s slots -- within noise, not bit for bit: rotate decomposes
    sigma_g(c1), this call c1 itself.  Needs the same keys (ckks.rotationKeyGen(rs)); indices
    may repeat, 0 is a copy, 1 <= R <= 64.  out must not overlap ct.  Scale unchanged."""
    torch = _torch()
    _check_ct(ct, ckks, any_level=True)
    rs = [int(r) for r in rs]
    R = len(rs)
    if not 1 <= R <= ROTATE_MANY_MAX:
        raise ValueError("rotate_many takes 1..%d rotation indices" % ROTATE_MANY_MAX)
    if any(not -(1 << 31) <= r < 1 << 31 for r in rs):
        raise ValueError("rotation index must be below the batch size")
    K, _, l, N = ct.shape
    if out is None:
        out = torch.empty((R, K, 2, l, N), dtype=ct.dtype, device=ct.device)
    if (not out.is_cuda or not out.is_contiguous() or out.element_size() != 8 or tuple(out.shape) != (R, K, 2, l, N)
            or out.device != ct.device):
        raise ValueError("out must be a contiguous [R][K][2][l][N] 64-bit tensor on ct's device")
    idx = (C.c_int32 * R)(*rs)
    check(_lib.load().shelfi_dev_rotate_many(ckks._ctx, C.c_void_p(ct.data_ptr()), K, int(l), idx, R,
                                             C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(ct))),
          "dev_rotate_many")
    return out


def diagonals(M):
    """The non-zero generalized diagonals of a batch x batch matrix, {d: M[s][(s + d) mod batch] over s}: the
    form lin_transform takes, y = M x being y[s] = sum_d diag_d[s] x[(s + d) mod batch]."""
    import numpy as np

    M = np.asarray(M, dtype=np.float64)
    if M.ndim != 2 or M.shape[0] != M.shape[1] or not M.shape[0]:
        raise ValueError("diagonals() needs a square matrix")
    n = M.shape[0]
    s = np.arange(n)
    out = {}
    for d in range(n):
        v = M[s, (s + d) % n]
        if v.any():
            out[d] = v.copy()
    return out


def _lin_plan(diags, babies=None):
    """The baby-step / giant-step plan of a set of diagonals {d: vector of batch values}: (batch, b, {G: {i: d}})
    with d = G + i (mod batch), 0 <= i < b and G a multiple of b.  The diagonal indices are taken modulo batch, as
    0 .. batch - 1 or centred on 0, whichever spans less (a band around the main diagonal is centred)."""
    import math

    if not hasattr(diags, "items") or not len(diags):
        raise ValueError("a linear transform needs a dict {diagonal index: vector of batch values}, not empty")
    batch = len(next(iter(diags.values())))
    if any(len(v) != batch for v in diags.values()):
        raise ValueError("every diagonal must hold batch values")
    up = sorted({int(d) % batch for d in diags})
    if len(up) != len(diags):
        raise ValueError("two diagonal indices are the same modulo batch")
    centred = sorted(d - batch if d > batch // 2 else d for d in up)
    reps = up if up[-1] - up[0] <= centred[-1] - centred[0] else centred
    span = reps[-1] - reps[0] + 1
    if babies is None:
        b = 1 << max(0, round(math.log2(math.sqrt(span))))
    else:
        b = int(babies)
        if b < 1 or b & (b - 1) or b > batch:
            raise ValueError("babies must be a power of two in 1..batch")
    plan = {}
    for d in reps:
        G = (d // b) * b
        plan.setdefault(G, {})[d - G] = d % batch
    return batch, b, plan


def lin_transform_indices(diags, babies=None):
    """The rotation indices lin_transform(ckks, ct, diags, babies=babies) needs keys for (rotationKeyGen's
    argument): the baby steps it takes in one rotate_many and the giant steps it takes by rotate.  A plan that
    needs more than the 64 keys a context holds is refused."""
    _, b, plan = _lin_plan(diags, babies)
    baby = sorted({i for steps in plan.values() for i in steps} - {0})
    giant = sorted(set(plan) - {0})
    keys = sorted(set(baby) | set(giant))
    if len(keys) > ROTATE_MANY_MAX:
        raise ValueError("this plan needs %d rotation keys, a context holds %d: babies b = %d with %d giant steps; "
                         "choose another babies" % (len(keys), ROTATE_MANY_MAX, b, len(plan)))
    return keys


def lin_transform(ckks, ct, diags, scale=None, babies=None, out=None):
    """A public batch x batch matrix applied to the slots of K ciphertexts [K][2][l][N], given by its diagonals
    {d: vector} (diagonals(M)): y[s] = sum_d diags[d][s] x[(s + d) mod batch], by baby steps and giant steps.
    One rotate_many makes the baby rotations x_i, i < b, from one decomposition; then per giant step G (a
    multiple of b) one dot_plain sums x_i (.) encode(roll(diags[G + i], G)) over i, one rotate by G turns it, and
    add collects the giants.  The plaintexts are encoded at `scale` (default q[l - 1]) and the sum is rescaled
    once: the result [K][2][l - 1][N] is at the input's scale.  babies: b, a power of two (default: the one
    nearest the square root of the diagonals' span).  Needs ckks.rotationKeyGen(lin_transform_indices(diags,
    babies)) and l >= 2; real slot packing only."""
    torch = _torch()
    _check_ct(ct, ckks, any_level=True)
    K, _, l, N = ct.shape
    inf = ckks.info()
    batch, b, plan = _lin_plan(diags, babies)
    lin_transform_indices(diags, babies)  # the 64-key limit, by name
    if batch != inf["batch"] or inf["values_per_ct"] != inf["batch"]:
        raise ValueError("the diagonals must hold batch = %d values (real slot packing)" % inf["batch"])
    if l < 2:
        raise ValueError("a linear transform spends one level: the input needs at least 2 towers")
    if K == 0:
        raise ValueError("a linear transform needs at least one ciphertext")
    scale = float(inf["moduli"][l - 1] if scale is None else scale)
    dg = {int(d) % batch: torch.as_tensor(v, dtype=torch.float64).to(ct.device) for d, v in diags.items()}
    baby = sorted({i for steps in plan.values() for i in steps})
    rots = rotate_many(ckks, ct, baby)  # [len(baby)][K][2][l][N]
    acc = None
    for G in sorted(plan):
        steps = sorted(plan[G])
        pts = encode(ckks, torch.cat([torch.roll(dg[plan[G][i]], G) for i in steps]).contiguous(), towers=l,
                     scale=scale)  # [len(steps)][l][N]
        sel = [baby.index(i) for i in steps]
        part = torch.empty_like(ct)
        for k in range(K):  # the plaintext step per ciphertext: its stacked baby rotations against the diagonals
            stack = rots[sel, k] if sel != list(range(len(baby))) else rots[:, k]
            dot_plain(ckks, stack.contiguous(), pts, out=part[k:k + 1])
        if G:
            part = rotate(ckks, part, G)
        acc = part if acc is None else add(ckks, acc, part, out=acc)
    return rescale(ckks, acc, out=out)


def conj(ckks, ct, out=None):
    """The complex conjugate of every slot of K ciphertexts of any level: the automorphism X -> X^(2N - 1) and
    its key switch, (sigma(c0) + u0, u1) with (u0, u1) = KeySwitch(sigma(c1)).  Needs ckks.conjugateKeyGen().
    out must not overlap ct.  Scale unchanged.  Under complex slot packing dot(u, conj(u)) is the squared norm,
    and (ct + conj(ct)) / 2 holds the even-indexed values alone."""
    _check_ct(ct, ckks, any_level=True)
    out = _like(ckks, ct, out)
    check(_lib.load().shelfi_dev_conjugate(ckks._ctx, C.c_void_p(ct.data_ptr()), ct.shape[0], int(ct.shape[2]),
                                           C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(ct))), "dev_conjugate")
    return out


def eval_sum(ckks, ct, n: int, out=None):
    """cc->EvalSum(ct, n), n a power of two in 1..batch: slot i of the result holds
    sum_{j < n} x[(i + j) mod batch], by log2(n) rotate-and-add steps (needs the keys of indices
    1, 2, .., n / 2: ckks.evalSumKeyGen()).  out must not overlap ct.  Scale unchanged."""
    _check_ct(ct, ckks, any_level=True)
    out = _like(ckks, ct, out)
    if n < 0 or n >= 1 << 32:
        raise ValueError("EvalSum needs a power of two in 1..batch")
    check(_lib.load().shelfi_dev_eval_sum(ckks._ctx, C.c_void_p(ct.data_ptr()), ct.shape[0], int(ct.shape[2]),
                                          int(n), C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(ct))),
          "dev_eval_sum")
    return out


def add(ckks, a, b, out=None):
    """cc->EvalAdd(a, b) for K ciphertext pairs of the same level and scale: out = a + b mod q_t
    (out may be a or b).  Needs no keys; enqueued on a's stream."""
    _check_ct(a, ckks, any_level=True)
    _check_ct(b, ckks, a.shape[0], any_level=True)
    if a.shape != b.shape or b.device != a.device:
        raise ValueError("EvalAdd operands must have the same shape (same level) and device")
    out = _like(ckks, a, out)
    check(_lib.load().shelfi_dev_add(ckks._ctx, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), a.shape[0],
                                     int(a.shape[2]), C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(a))),
          "dev_add")
    return out


def sub(ckks, a, b, out=None):
    """cc->EvalSub(a, b) for K ciphertext pairs of the same level and scale: out = a - b mod q_t
    (out may be a or b).  Needs no keys; enqueued on a's stream."""
    _check_ct(a, ckks, any_level=True)
    _check_ct(b, ckks, a.shape[0], any_level=True)
    if a.shape != b.shape or b.device != a.device:
        raise ValueError("EvalSub operands must have the same shape (same level) and device")
    out = _like(ckks, a, out)
    check(_lib.load().shelfi_dev_sub(ckks._ctx, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), a.shape[0],
                                     int(a.shape[2]), C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(a))),
          "dev_sub")
    return out


def neg(ckks, ct, out=None):
    """cc->EvalNegate(ct): out = -ct mod q_t (out may be ct).  Needs no keys; enqueued on ct's stream."""
    _check_ct(ct, ckks, any_level=True)
    out = _like(ckks, ct, out)
    check(_lib.load().shelfi_dev_negate(ckks._ctx, C.c_void_p(ct.data_ptr()), ct.shape[0], int(ct.shape[2]),
                                        C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(ct))), "dev_negate")
    return out


def encode(ckks, x, towers=None, scale=None, out=None):
    """cc->MakeCKKSPackedPlaintext without the Encrypt: a float64 CUDA vector of n values -> K =
    ceil(n / batch) plaintexts, an int64 tensor [K][towers][N] (EVALUATION, canonical residues), by the
    encode inside encrypt exactly.  towers defaults to L and scale to the context's delta (an operand
    for add_plain / sub_plain on a fresh ciphertext); a factor for mult_plain whose product is to be
    rescale()d back to the ciphertext's scale is encoded at scale=float(q[towers - 1]).  A coefficient
    above 2^61 in magnitude, or a non-finite value, raises ValueError.  Needs no keys."""
    torch = _torch()
    if not x.is_cuda or x.dtype != torch.float64 or not x.is_contiguous():
        raise ValueError("x must be a contiguous float64 CUDA tensor")
    inf = ckks.info()
    L, N, B = inf["num_towers"], inf["ring_dim"], inf["values_per_ct"]
    towers = L if towers is None else int(towers)
    scale = float(inf["delta"] if scale is None else scale)
    if not 0 <= towers < 1 << 32:
        raise ValueError("tower count out of range for this context")
    K = (x.numel() + B - 1) // B
    if out is None:
        out = torch.empty((K, max(towers, 0), N), dtype=torch.int64, device=x.device)
    if (not out.is_cuda or not out.is_contiguous() or out.element_size() != 8 or tuple(out.shape) != (K, towers, N)
            or out.device != x.device):
        raise ValueError("out must be a contiguous [K][towers][N] 64-bit tensor on x's device")
    check(_lib.load().shelfi_dev_encode(ckks._ctx, C.c_void_p(x.data_ptr()), x.numel(), towers, scale,
                                        C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(x))), "dev_encode")
    return out


def _plain_op(fn, what, ckks, ct, pt, out):
    _check_ct(ct, ckks, any_level=True)
    K, _, l, N = ct.shape
    if not pt.is_cuda or not pt.is_contiguous() or pt.element_size() != 8 or pt.device != ct.device:
        raise ValueError("plaintext tensors must be contiguous 64-bit CUDA tensors on the ciphertexts' device")
    sh = tuple(pt.shape)
    if len(sh) == 2:  # one plaintext [towers][N] for every ciphertext
        sh = (1,) + sh
    if len(sh) != 3 or sh[1:] != (l, N) or sh[0] not in (1, K):
        raise ValueError("plaintext tensor must have shape [K][towers][N] = [%d][%d][%d], or hold one plaintext"
                         % (K, l, N))
    out = _like(ckks, ct, out)
    check(fn(ckks._ctx, C.c_void_p(ct.data_ptr()), C.c_void_p(pt.data_ptr()), K, sh[0], int(l),
             C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(ct))), what)
    return out


def mult_plain(ckks, ct, pt, out=None):
    """cc->EvalMult(ct, pt): both components of K ciphertexts [K][2][l][N] times the plaintexts pt
    [K][l][N] (or one plaintext, [1][l][N] or [l][N], for every ciphertext); out may be ct.  Scale:
    scale_ct * scale_pt.  Needs no keys; enqueued on ct's stream."""
    return _plain_op(_lib.load().shelfi_dev_mult_plain, "dev_mult_plain", ckks, ct, pt, out)


def add_plain(ckks, ct, pt, out=None):
    """cc->EvalAdd(ct, pt): c0 + pt, c1 unchanged; pt as for mult_plain, at the ciphertext's scale."""
    return _plain_op(_lib.load().shelfi_dev_add_plain, "dev_add_plain", ckks, ct, pt, out)


def sub_plain(ckks, ct, pt, out=None):
    """cc->EvalSub(ct, pt): c0 - pt, c1 unchanged; pt as for mult_plain, at the ciphertext's scale."""
    return _plain_op(_lib.load().shelfi_dev_sub_plain, "dev_sub_plain", ckks, ct, pt, out)


PROJECT_MAX_BATCHES = 32  # shelfi_dev_project: as GRAM_MAX_BATCHES, for the ciphertext and the plaintext side


def project(ckks, batches, pts, out=None):
    """cc->EvalInnerProduct(ct, pt) for every pair of C ciphertext batches and R plaintext batches at one level:
    a batch [C R][2][l][N] whose entry c R + r is sum_k batches[c][k] (.) pts[r][k] in both components -- its
    slots hold sum_k x_ck[s] g_rk[s], the projection of update c on the known vector r before the sum over slots
    (rescale, then eval_sum).  Needs no key of any kind.  batches: a sequence of 1..32 tensors [K][2][l][N] (the
    same tensor may appear twice), or one stacked [C][K][2][l][N] tensor; pts: [R][K][l][N] with 1 <= R <= 32, or
    [K][l][N] for R = 1, as device.encode writes them.  out must overlap no input.  Scale: scale_ct * scale_pt.
    At C = R = K = 1 the result is mult_plain's, bit for bit."""
    torch = _torch()
    if hasattr(batches, "dim"):
        if batches.dim() != 5 or not batches.is_contiguous():
            raise ValueError("a stacked EvalInnerProduct operand must be a contiguous [C][K][2][l][N] tensor")
        batches = [batches[i] for i in range(batches.shape[0])]
    batches = list(batches)
    n = len(batches)
    if not 1 <= n <= PROJECT_MAX_BATCHES:
        raise ValueError("EvalInnerProduct(ct, pt) needs 1..%d ciphertext batches" % PROJECT_MAX_BATCHES)
    a = batches[0]
    _check_ct(a, ckks, any_level=True)
    for b in batches[1:]:
        _check_ct(b, ckks, a.shape[0], any_level=True)
        if b.shape != a.shape:
            raise ValueError("EvalInnerProduct(ct, pt) operands must have the same shape (same level)")
        if b.device != a.device:
            raise ValueError("EvalInnerProduct(ct, pt) operands must live on the same device")
    K, _, l, N = a.shape
    if K == 0:  # (an empty tensor has no storage to hand the library, which refuses K = 0 by name)
        raise ValueError("EvalInnerProduct(ct, pt) needs at least one ciphertext a batch")
    if not hasattr(pts, "dim") or not pts.is_cuda or not pts.is_contiguous() or pts.element_size() != 8 or pts.device != a.device:
        raise ValueError("plaintext tensors must be contiguous 64-bit CUDA tensors on the ciphertexts' device")
    sh = tuple(pts.shape)
    if len(sh) == 3:  # one plaintext batch [K][l][N]
        sh = (1,) + sh
    if len(sh) != 4 or sh[1:] != (K, l, N):
        raise ValueError("plaintext tensor must have shape [R][K][towers][N] = [R][%d][%d][%d], or hold one batch"
                         % (K, l, N))
    R = sh[0]
    if not 1 <= R <= PROJECT_MAX_BATCHES:
        raise ValueError("EvalInnerProduct(ct, pt) needs 1..%d plaintext batches" % PROJECT_MAX_BATCHES)
    if out is None:
        out = torch.empty((n * R, 2, l, N), dtype=a.dtype, device=a.device)
    _check_ct(out, ckks, n * R, any_level=True)
    if tuple(out.shape) != (n * R, 2, l, N) or out.device != a.device:
        raise ValueError("out must be a contiguous [C R][2][l][N] 64-bit tensor on the batches' device")
    ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in batches])
    check(_lib.load().shelfi_dev_project(ckks._ctx, ptrs, n, C.c_void_p(pts.data_ptr()), R, K, int(l),
                                         C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(a))), "dev_project")
    return out


def dot_plain(ckks, ct, pt, out=None):
    """cc->EvalInnerProduct(ct, pt): sum_k ct[k] (.) pt[k] over K ciphertexts [K][2][l][N] and K plaintexts
    [K][l][N] -> one ciphertext [1][2][l][N]; project() at C = R = 1."""
    if hasattr(pt, "dim") and pt.dim() != 3:
        raise ValueError("plaintext tensor must have shape [K][towers][N]")
    return project(ckks, [ct], pt, out=out)


def _one_hots(ckks, l: int, P: int, device):
    """The P one-hot slot vectors e_p as plaintexts [P][l][N] at scale q[l - 1], cached on the context per
    (l, P, device) and parameter generation.  The same plaintexts in either slot packing: vector p spans the V
    values of one plaintext and its 1.0 is the real part of slot p (value p, or 2 p under complex packing)."""
    torch = _torch()
    gen = getattr(ckks, "_params_gen", 0)
    cache = getattr(ckks, "_dev_one_hots", None)
    if cache is None or cache[0] != gen:
        cache = ckks._dev_one_hots = (gen, {})
    key = (int(l), int(P), str(device))
    if key not in cache[1]:
        inf = ckks.info()
        V = inf["values_per_ct"]
        x = torch.zeros(P * V, dtype=torch.float64, device=device)
        x[torch.arange(P, device=device) * (V + V // inf["batch"])] = 1.0
        cache[1][key] = encode(ckks, x, towers=l, scale=float(inf["moduli"][l - 1]))
    return cache[1][key]


def pack_slots(ckks, cts, out=None):
    """P ciphertexts that each hold one number in every slot (eval_sum's output: the entries of a Gram matrix,
    projections) -> ONE ciphertext [1][2][l-1][N] whose slot p holds slot p of cts[p], p < P, and 0 elsewhere:
    sum_p cts[p] (.) e_p with the one-hot plaintexts e_p encoded at scale q[l - 1] (dot_plain), then rescale --
    one decrypt, or one partial decryption a party, opens all P numbers.  cts: [P][2][l][N], 1 <= P <= batch,
    l >= 2.  Needs no key; the scale stays the inputs' own; one level is spent."""
    _check_ct(cts, ckks, any_level=True)
    P, _, l, N = cts.shape
    if l < 2:
        raise ValueError("pack_slots needs at least 2 towers (it ends in a ModReduce)")
    if not 1 <= P <= ckks.info()["batch"]:
        raise ValueError("pack_slots takes 1..batch ciphertexts, one a slot")
    return rescale(ckks, dot_plain(ckks, cts, _one_hots(ckks, l, P, cts.device)), out=out)


def ntt(ckks, polys, inverse: bool = False):
    """In-place negacyclic NTT (PALISADE order) of [P][N] polys; tower = p % L.  Inputs are canonical
    residues below their tower's modulus, outputs are canonical, and P may be any count."""
    inf = ckks.info()
    if not polys.is_cuda or not polys.is_contiguous() or polys.shape[-1] != inf["ring_dim"]:
        raise ValueError("polys must be a contiguous CUDA tensor [P][N]")
    # the kernels transform P polynomials of 8-byte words: any other element size is a shorter buffer
    if polys.dtype != _torch().int64 or polys.numel() % inf["ring_dim"]:
        raise ValueError("polys must be int64 (uint64 residues), a whole number of polynomials")
    P = polys.numel() // inf["ring_dim"]
    check(_lib.load().shelfi_dev_ntt(ckks._ctx, C.c_void_p(polys.data_ptr()), P, 1 if inverse else 0,
                                     C.c_void_p(_stream_ptr(polys))), "dev_ntt")
    return polys


def encrypt_seeded(ckks, x):
    """The symmetric encrypt of a float64 CUDA vector into K = ceil(n / batch) seeded ciphertexts
    (DESIGN.md §2.17): (c0, seed) with c0 an int64 tensor [K][L][N] and seed the call's 32 public bytes;
    expand_seeded(ckks, c0, seed) is the ordinary batch.  Needs the whole secret key (not a threshold
    share); a coefficient above 2^61 in magnitude, or a non-finite value, raises ValueError."""
    torch = _torch()
    if not x.is_cuda or x.dtype != torch.float64:
        raise ValueError("x must be a float64 CUDA tensor")
    x = x.contiguous().view(-1)
    inf = ckks.info()
    K = (x.numel() + inf["values_per_ct"] - 1) // inf["values_per_ct"]
    c0 = torch.empty((K, inf["num_towers"], inf["ring_dim"]), dtype=torch.int64, device=x.device)
    seed = (C.c_uint8 * 32)()
    check(_lib.load().shelfi_dev_encrypt_seeded(ckks._ctx, C.c_void_p(x.data_ptr()), x.numel(),
                                                C.c_void_p(c0.data_ptr()), seed, C.c_void_p(_stream_ptr(x))),
          "dev_encrypt_seeded")
    return c0, bytes(seed)


def expand_seeded(ckks, c0, seed: bytes, k0: int = 0, out=None):
    """c0 [K][l][N] (l <= L towers) and a 32-byte seed -> the batch [K][2][l][N]: polynomial 0 is c0,
    polynomial 1 the seed's stream of ciphertexts k0 .. k0 + K - 1 (k0: the first one's index in its
    blob).  An ordinary batch for Arena.put, wavg, decrypt and the rest."""
    torch = _torch()
    L, N = _ln(ckks)
    if (not c0.is_cuda or not c0.is_contiguous() or c0.dtype != torch.int64 or c0.dim() != 3 or c0.shape[2] != N
            or not 1 <= c0.shape[1] <= L):
        raise ValueError("c0 must be a contiguous int64 CUDA tensor [K][l][N] with l <= L")
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("the seed is 32 bytes")
    if not 0 <= int(k0) < 1 << 48:
        raise ValueError("ciphertext index at or above 2^48")
    K, l = int(c0.shape[0]), int(c0.shape[1])
    if out is None:
        out = torch.empty((K, 2, l, N), dtype=torch.int64, device=c0.device)
    if (not out.is_cuda or not out.is_contiguous() or out.dtype != torch.int64 or tuple(out.shape) != (K, 2, l, N)
            or out.device != c0.device):
        raise ValueError("out must be a contiguous int64 [K][2][l][N] tensor on c0's device")
    out[:, 0].copy_(c0)
    check(_lib.load().shelfi_dev_expand_seeded(ckks._ctx, C.c_void_p(out.data_ptr()), K, l,
                                               (C.c_uint8 * 32).from_buffer_copy(seed), int(k0),
                                               C.c_void_p(_stream_ptr(out))), "dev_expand_seeded")
    return out


def from_blob(ckks, blob, out=None):
    """Ciphertext bytes in any wire format -> the [K][2][L][N] batch on the device: a packed blob is
    unpacked and a seeded blob's c1 expanded there (the host cannot: blob_residues refuses one)."""
    import numpy as np

    from . import blob_info

    K = blob_info(bytes(blob))["num_cts"]
    if out is None:
        out = empty_ct(ckks, K)
    _check_ct(out, ckks, K)
    host = np.frombuffer(blob, dtype=np.uint8)
    check(_lib.load().shelfi_dev_blob_unpack(ckks._ctx, C.c_void_p(host.ctypes.data), host.size, K,
                                             C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(out))),
          "dev_blob_unpack")
    return out


def from_bytes(ckks, blob: bytes, device=None):
    """Blob payload -> device ciphertext tensor (one H2D copy)."""
    import numpy as np

    from . import blob_residues

    torch = _torch()
    inf = ckks.info()
    arr = blob_residues(blob, inf["ring_dim"], inf["num_towers"]).view(np.int64)
    if device is None:
        device = "cuda:%d" % inf["device"]
    return torch.from_numpy(arr.copy()).to(device)
