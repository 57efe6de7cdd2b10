#!/usr/bin/env python3
"""Time D.rotate, D.mult and D.eval_sum(., batch) in one process.

Shape: ring 2^15, 4 towers (two full digits), K = 714 ciphertexts -- one cfg3 learner, the shape
EvalMult is measured at.  Each call ends in the library's own stream synchronise, so a host clock around it is a device
time plus one launch chain.  Every shape is warmed up first; the three operations alternate inside
every round, so drift hits them alike; the spread of the mult rounds is the yardstick a rotation is
read against (it runs mult's key switch behind a lighter first pass).

Prints one JSON line: microseconds per ciphertext, median and [min, max] over the rounds.
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
    ap.add_argument("--cts", type=int, default=714)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="mult / rotate calls per round")
    a = ap.parse_args()

    import torch

    import SHELFI_FHE as m
    from SHELFI_FHE import device as D

    if not torch.cuda.is_available():
        sys.exit("rotate_bench needs a GPU: there is no CPU timing to report")
    c = m.CKKS("ckks", a.batch, 52, "", multDepth=a.depth, seed=7, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    c.evalMultKeyGen()
    c.evalSumKeyGen()
    inf = c.info()
    S, K = inf["batch"], a.cts
    x = torch.rand(K * S, dtype=torch.float64, device="cuda") * 2 - 1
    ct = D.encrypt(c, x)
    out = torch.empty_like(ct)

    def timed(f, reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps / K * 1e6

    ops = {
        "mult": (lambda: D.mult(c, ct, ct, out=out), a.reps),
        "rotate": (lambda: D.rotate(c, ct, 1, out=out), a.reps),
        "eval_sum": (lambda: D.eval_sum(c, ct, S, out=out), 1),
    }
    for f, _ in ops.values():  # warm-up: code objects, level tables, scratch
        f()
        f()
    us = {k: [] for k in ops}
    for _ in range(a.rounds):
        for k, (f, reps) in ops.items():
            us[k].append(timed(f, reps))
    res = {"ring_dim": inf["ring_dim"], "towers": inf["num_towers"], "batch": S, "cts": K, "rounds": a.rounds,
           "eval_sum_rotations": S.bit_length() - 1}
    for k, v in us.items():
        res[k + "_us_per_ct"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
                                 "max": round(max(v), 3)}
    res["rotate_over_mult"] = round(statistics.median(us["rotate"]) / statistics.median(us["mult"]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
