#!/usr/bin/env python3
"""Threshold CKKS on the device, microseconds per ciphertext at cfg3 (2^15 / L4, K = 714, one ResNet-18
learner), steady state: partial_decrypt (lead and main, sigma = 0 and 2^20), fuse_decrypt at P = 2, 3 and
16 and device.decrypt on the same ciphertexts in the same process.  One JSON line.

Each figure is the median over --rounds rounds of one call timed with device events on the call's
stream, the variants interleaved inside a round so drift hits them alike; the calls synchronise their
stream themselves, so a call's launch gaps are inside its figure (a few us against milliseconds).
`floor_us_per_ct` is each call's compulsory HBM traffic over 6.4 TB/s (the aggregation kernel's rate): what the
element-wise partial decryption should approach.  --decrypt-only times device.decrypt alone (for a run
under SHELFI_LIB_AB with a build that lacks the threshold entry points: the parent-commit comparison).

  python tools/threshold_bench.py [--K 714] [--rounds 9] [--decrypt-only]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-fed_amd"))
import torch  # noqa: E402

import SHELFI_FHE as m  # noqa: E402
from SHELFI_FHE import device as D  # noqa: E402

BATCH, DEPTH = 16384, 3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=714)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--decrypt-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("threshold_bench: no GPU (there is no CPU path to time)")
    K = a.K
    ck = m.CKKS("ckks", BATCH, 52, "", multDepth=DEPTH, seed=7, decodeNoise=False)
    assert ck.genCryptoContextAndKeyGen() == 1
    inf = ck.info()
    L, N, delta = inf["num_towers"], inf["ring_dim"], inf["delta"]
    n = K * BATCH
    x = torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1
    ct = D.encrypt(ck, x)
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    runs = {"decrypt": lambda: D.decrypt(ck, ct, n, delta, out=out)}
    poly = L * N * 8  # bytes of one polynomial over every tower
    floor = {}
    if not a.decrypt_only:
        pout = torch.empty((K, L, N), dtype=torch.int64, device="cuda")
        # 16 distinct partial buffers (the same address twice would be served by the caches): the lead's
        # under the whole key and 15 of zeros, so the fused value is the ciphertexts' plaintext and the
        # call stays on decrypt's fast path (partials that sum to noise send every call to the exact redo)
        ck.set_threshold_noise(0.0)
        parts = [D.partial_decrypt(ck, ct, True)] + [torch.zeros((K, L, N), dtype=torch.int64, device="cuda")
                                                     for _ in range(15)]

        def pd(lead, sigma):
            def f():
                ck.set_threshold_noise(sigma)
                D.partial_decrypt(ck, ct, lead, out=pout)
            return f

        for lead in (True, False):
            for sigma, tag in ((0.0, "s0"), (2.0 ** 20, "s2p20")):
                name = "partial_%s_%s" % ("lead" if lead else "main", tag)
                runs[name] = pd(lead, sigma)
                floor[name] = (3 if lead else 2) * poly / 6.4e6  # the key's {s, s'} are shared: caches
        for P in (2, 3, 16):
            runs["fuse_P%d" % P] = (lambda P: lambda: D.fuse_decrypt(ck, parts[:P], n, delta, out=out))(P)
    for f in runs.values():  # warm every shape
        f()
        f()
    torch.cuda.synchronize()
    if not a.decrypt_only:  # what is timed is the right result
        ref = D.decrypt(ck, ct, n, delta).clone()
        redo = ck.decode_redo_count()
        for P in (2, 3, 16):
            assert torch.equal(D.fuse_decrypt(ck, parts[:P], n, delta), ref), "fuse differs from decrypt"
        assert ck.decode_redo_count() == redo, "a timed call left the fast path"
    t = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, f in runs.items():
            t[k].append(timed(f))
    res = {"tool": "threshold_bench", "K": K, "ring_dim": N, "towers": L, "rounds": a.rounds,
           "us_per_ct": {k: round(statistics.median(v) / K, 3) for k, v in t.items()},
           "us_per_ct_min": {k: round(min(v) / K, 3) for k, v in t.items()},
           "us_per_ct_max": {k: round(max(v) / K, 3) for k, v in t.items()},
           "floor_us_per_ct": {k: round(v, 3) for k, v in floor.items()},
           "lib": os.environ.get("SHELFI_LIB_AB", "in-tree")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
