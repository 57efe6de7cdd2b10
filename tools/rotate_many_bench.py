#!/usr/bin/env python3
"""Time D.rotate_many against R D.rotate calls, and D.lin_transform against its term-by-term composition, in one
process.

Shape: ring 2^15, 4 towers (two full digits), K in {1, 64, 714} ciphertexts, R in {2, 4, 8, 16} rotations of
indices 1 .. R.  Each call ends in the library's own stream synchronise, so a host clock around it is a device time
plus its launch chains.  Every shape is warmed up first; the two sides alternate inside every round, so drift hits
them alike.  The linear transform has 16 diagonals (0 .. 15, uniform entries): lin_transform's plan (babies 4: one
rotate_many of 1 .. 3, four dot_plain, three rotate, one rescale) against sum_d mult_plain(rotate(ct, d),
encode(diag_d)), added term by term and rescaled once.

SHELFI_HOIST_KEYS_PER_PASS (read once a process) sets how many rotations one workgroup of the hoisted inner product
serves; the value in force is reported.

Prints one JSON line per K: microseconds per ciphertext, median and [min, max] over the rounds.
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
    ap.add_argument("--cts", type=int, nargs="+", default=[1, 64, 714])
    ap.add_argument("--rotations", type=int, nargs="+", default=[2, 4, 8, 16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--diagonals", type=int, default=16, help="0 skips the linear transform")
    a = ap.parse_args()

    import torch

    import SHELFI_FHE as m
    from SHELFI_FHE import device as D

    if not torch.cuda.is_available():
        sys.exit("rotate_many_bench needs a GPU: there is no CPU timing to report")
    c = m.CKKS("ckks", a.batch, 52, "", multDepth=a.depth, seed=7, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    S, l = inf["batch"], inf["num_towers"]
    Rmax = max(a.rotations + [a.diagonals - 1])
    c.rotationKeyGen(range(1, Rmax + 1))
    diags = {d: torch.rand(S, dtype=torch.float64, device="cuda") * 2 - 1 for d in range(a.diagonals)}
    ql = float(inf["moduli"][l - 1])

    def med(v):
        return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}

    for K in a.cts:
        x = torch.rand(K * S, dtype=torch.float64, device="cuda") * 2 - 1
        ct = D.encrypt(c, x)
        reps = 5 if K >= 64 else 50

        def timed(f, n=reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(n):
                f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n / K * 1e6

        res = {"ring_dim": inf["ring_dim"], "towers": l, "batch": S, "cts": K, "rounds": a.rounds,
               "keys_per_pass": int(os.environ.get("SHELFI_HOIST_KEYS_PER_PASS", "0")) or "default"}
        for R in a.rotations:
            rs = list(range(1, R + 1))
            out = torch.empty((R,) + tuple(ct.shape), dtype=ct.dtype, device="cuda")

            def singles():
                for i, r in enumerate(rs):
                    D.rotate(c, ct, r, out=out[i])

            def many():
                D.rotate_many(c, ct, rs, out=out)

            for f in (singles, many, singles, many):  # warm-up: code objects, level tables, scratch
                f()
            us = {"rotate": [], "rotate_many": []}
            for _ in range(a.rounds):
                us["rotate"].append(timed(singles))
                us["rotate_many"].append(timed(many))
            res["R%d" % R] = {
                "rotate_us_per_ct": med(us["rotate"]), "rotate_many_us_per_ct": med(us["rotate_many"]),
                "per_rotation_us": round(statistics.median(us["rotate_many"]) / R, 3),
                "many_over_rotate": round(statistics.median(us["rotate_many"]) / statistics.median(us["rotate"]), 4)}
            del out
        if a.diagonals:
            def bsgs():
                return D.lin_transform(c, ct, diags)

            def terms():
                acc = None
                for d, v in diags.items():
                    pt = D.encode(c, v, towers=l, scale=ql)
                    t = D.mult_plain(c, D.rotate(c, ct, d), pt)
                    acc = t if acc is None else D.add(c, acc, t, out=acc)
                return D.rescale(c, acc)

            for f in (bsgs, terms):
                f()
            us = {"lin_transform": [], "term_by_term": []}
            for _ in range(a.rounds):
                us["lin_transform"].append(timed(bsgs, 2))
                us["term_by_term"].append(timed(terms, 2))
            res["lin_transform_%d" % a.diagonals] = {
                "lin_transform_us_per_ct": med(us["lin_transform"]), "term_by_term_us_per_ct": med(us["term_by_term"]),
                "ratio": round(statistics.median(us["lin_transform"]) / statistics.median(us["term_by_term"]), 4)}
        print(json.dumps(res), flush=True)
        del ct, x


if __name__ == "__main__":
    main()
