#!/usr/bin/env python3
"""Time multiEvalSumKeyGen beside evalSumKeyGen in one process.

Shape: ring 2^15, 4 towers, batch 16384 -- 14 rotation keys per call.  Every call ends in the
library's own stream synchronise, so a host clock around it is device time plus the call's host work:
evalSumKeyGen also installs its keys (Shoup companions on the host, two uploads per key); a share
call returns its keys to the host instead, and a follower's uploads the previous party's first.  The
three calls alternate inside every round, so drift hits them alike.

Prints one JSON line: milliseconds per call, median and [min, max] over the rounds.
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
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()

    import torch

    import SHELFI_FHE as m

    if not torch.cuda.is_available():
        sys.exit("multikey_bench needs a GPU: there is no CPU timing to report")
    c = m.CKKS("ckks", a.batch, 52, "", multDepth=a.depth, seed=7, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    prev = c.multiEvalSumKeyGen()

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    ops = {
        "eval_sum_keygen": c.evalSumKeyGen,
        "multi_eval_sum_keygen_lead": c.multiEvalSumKeyGen,
        "multi_eval_sum_keygen_follower": lambda: c.multiEvalSumKeyGen(prev),
    }
    for f in ops.values():  # warm-up: code objects, level tables, scratch
        f()
    ms = {k: [] for k in ops}
    for _ in range(a.rounds):
        for k, f in ops.items():
            ms[k].append(timed(f))
    res = {"ring_dim": inf["ring_dim"], "towers": inf["num_towers"], "batch": inf["batch"], "keys": len(prev),
           "key_mib": round(next(iter(prev.values())).nbytes / 2 ** 20, 2), "rounds": a.rounds}
    for k, v in ms.items():
        res[k + "_ms"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
