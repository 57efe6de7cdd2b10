#!/usr/bin/env python3
"""Time the bytes-API aggregation on seeded inputs against packed ones, in one process.

Shape: bench.py's bytes-API sample -- 16 learners x 64 ciphertexts, ring 2^15, 4 towers, the blobs made by
CKKS.encrypt in each format and aggregated by CKKS.computeWeightedAverage (H2D + unpack [+ c1 expansion] +
wavg + pack + D2H).  After a warm-up the two formats alternate inside every round, so drift hits them alike;
a round's figure is the median of its calls.  Also: microseconds per ciphertext of the symmetric encrypt
(D.encrypt_seeded) beside D.encrypt's, alternating the same way.

Prints one JSON line: per format client-ciphertexts/s and upload GB/s (median over the rounds, with the
rounds' [min, max]: each format's own spread), the ratio seeded / packed, and `seeded_not_slower`: seeded's
median rate is no more than packed's spread between repeats below packed's median.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-fed_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--learners", type=int, default=16)
    ap.add_argument("--cts", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5, help="aggregations per format per round")
    a = ap.parse_args()

    import numpy as np
    import torch

    import SHELFI_FHE as m
    from SHELFI_FHE import device as D

    if not torch.cuda.is_available():
        sys.exit("seeded_wire_bench needs a GPU: there is no CPU timing to report")
    c = m.CKKS("ckks", a.batch, 52, "", multDepth=a.depth, seed=7, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    S, L, N = inf["batch"], inf["num_towers"], inf["ring_dim"]
    C, K = a.learners, a.cts
    w = [1.0 / C] * C
    x = np.random.default_rng(7).uniform(-1, 1, K * S)
    blobs = {}
    for fmt in ("packed", "seeded"):
        c.set_wire_format(fmt)
        blobs[fmt] = [c.encrypt(x) for _ in range(C)]
    c.set_wire_format("shelfi")

    def stat(vals):
        return {"median": round(statistics.median(vals), 2), "min": round(min(vals), 2), "max": round(max(vals), 2)}

    def agg_ms(fmt):
        ts, kept = [], []  # every result is kept until its clock stops, as bench.py keeps them
        for _ in range(a.calls):
            t = time.perf_counter()
            kept.append(c.computeWeightedAverage(blobs[fmt], w))
            ts.append(time.perf_counter() - t)
        return statistics.median(ts) * 1e3

    for fmt in blobs:  # warm-up: staging rings, io buffers, code objects
        agg_ms(fmt)
    ms = {fmt: [] for fmt in blobs}
    for _ in range(a.rounds):
        for fmt in blobs:
            ms[fmt].append(agg_ms(fmt))
    res = {"ring_dim": N, "towers": L, "learners": C, "cts": K, "rounds": a.rounds, "calls": a.calls, "formats": {}}
    for fmt, v in ms.items():
        nb = sum(len(b) for b in blobs[fmt])
        res["formats"][fmt] = {"bytes_per_ct": (len(blobs[fmt][0]) - (128 if fmt == "seeded" else 64)) // K,
                               "ms_per_call": stat(v),
                               "client_cts_per_s": stat([C * K / (t * 1e-3) for t in v]),
                               "upload_GB_per_s": stat([nb / (t * 1e-3) / 1e9 for t in v])}
    pk, sd = res["formats"]["packed"]["client_cts_per_s"], res["formats"]["seeded"]["client_cts_per_s"]
    res["seeded_over_packed"] = round(sd["median"] / pk["median"], 3)
    res["packed_spread_cts_per_s"] = round(pk["max"] - pk["min"], 1)
    res["seeded_not_slower"] = bool(sd["median"] >= pk["median"] - (pk["max"] - pk["min"]))

    # the encrypts, per ciphertext, on the device API
    xd = torch.from_numpy(x).cuda()
    out = D.empty_ct(c, K)

    def timed(f, reps=5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps / K * 1e6

    ops = {"encrypt": lambda: D.encrypt(c, xd, out=out), "encrypt_seeded": lambda: D.encrypt_seeded(c, xd)}
    for f in ops.values():
        f()
    us = {k: [] for k in ops}
    for _ in range(a.rounds):
        for k, f in ops.items():
            us[k].append(timed(f))
    res["encrypt_us_per_ct"] = {k: stat(v) for k, v in us.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
