#!/usr/bin/env python3
"""Time D.gram against the loop of D.dot calls it replaces, in one process.

Shape: ring 2^15, 4 towers; C = 16 learners of K = 714 ciphertexts (cfg3) and C = 4 of K = 16.  For each shape,
alternating inside every round so drift hits them alike:

  gram      D.gram over the C batches                         P = C (C + 1) / 2 results, one key switch of P
  loop      D.dot(u_i, u_j) for every i <= j into slices of one output tensor: the path before gram, P key
            switches of one ciphertext each
  mult_p    D.mult over P ciphertext pairs: the batched key switch's share of gram
  dot_k1    D.dot on one pair of one ciphertext: the tail every dot of the loop ends in

Each call ends in the library's own stream synchronise, so a host clock around it is a device time plus its
launch chains.  Prints one JSON line: microseconds per call, median and [min, max] over the rounds; the bytes
each partial pass reads (gram: every tile's learners once; loop: both operands of a pair, one on the diagonal)
over the call's time and over the call's time less its measured tail; P, the slices and chains gram took; and
the bound gram is held to: loop - 0.8 (P dot_k1 - mult_p), at least 80% of what the single key switch saves.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-fed_amd"))

TILE = 2  # kGramTile


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="+", default=[16, 714, 4, 16], help="C K [C K ...]")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3, help="calls per round")
    a = ap.parse_args()

    import torch

    import SHELFI_FHE as m
    from SHELFI_FHE import device as D

    if not torch.cuda.is_available():
        sys.exit("gram_bench needs a GPU: there is no CPU timing to report")
    c = m.CKKS("ckks", a.batch, 52, "", multDepth=a.depth, seed=7, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    c.evalMultKeyGen()
    inf = c.info()
    S, L, N = inf["batch"], inf["num_towers"], inf["ring_dim"]
    shapes = list(zip(a.shapes[0::2], a.shapes[1::2]))
    Cmax, Kmax = max(s[0] for s in shapes), max(s[1] for s in shapes)
    us = [D.encrypt(c, torch.rand(Kmax * S, dtype=torch.float64, device="cuda") * 2 - 1) for _ in range(Cmax)]
    one = torch.empty((1, 2, L, N), dtype=torch.int64, device="cuda")

    def timed(f, reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps * 1e6

    def stat(vals):
        return {"median": round(statistics.median(vals), 2), "min": round(min(vals), 2), "max": round(max(vals), 2)}

    res = {"ring_dim": N, "towers": L, "rounds": a.rounds, "reps": a.reps, "shapes": {}}
    ct_bytes = 2 * L * N * 8
    for n, K in shapes:
        pairs = D.gram_pairs(n)
        P = len(pairs)
        bs = [u[:K] for u in us[:n]]
        G, Gl = (torch.empty((P, 2, L, N), dtype=torch.int64, device="cuda") for _ in range(2))
        assert P <= Kmax, "mult_p takes its P pairs from two learners' batches"
        x, y = us[0][:P], us[-1][:P]
        prod = torch.empty_like(x)

        def loop():
            for p, (i, j) in enumerate(pairs):
                D.dot(c, bs[i], bs[j], out=Gl[p:p + 1])

        ops = {
            "gram": lambda: D.gram(c, bs, out=G),
            "loop": loop,
            "mult_p": lambda: D.mult(c, x, y, out=prod),
            "dot_k1": lambda: D.dot(c, us[0][:1], us[-1][:1], out=one),
        }
        for f in ops.values():  # warm-up: code objects, level tables, scratch
            f()
            f()
        assert torch.equal(G, Gl), "gram differs from the loop of dots"
        us_ = {k: [] for k in ops}
        for _ in range(a.rounds):
            for k, f in ops.items():
                us_[k].append(timed(f, a.reps))
        r = {k + "_us": stat(w) for k, w in us_.items()}
        med = {k: statistics.median(w) for k, w in us_.items()}
        ops["gram"]()
        nt = -(-n // TILE)
        # gram reads a tile's learners once: 2 batches on the diagonal (1 when ragged), up to 4 off it
        gram_read = sum((min(TILE, n - i * TILE) + (min(TILE, n - j * TILE) if j != i else 0)) * K * ct_bytes
                        for i in range(nt) for j in range(i, nt))
        loop_read = sum((1 if i == j else 2) * K * ct_bytes for i, j in pairs)
        saving = P * med["dot_k1"] - med["mult_p"]
        r.update({
            "pairs": P, "slices": c.gram_slice_count(), "chains": c.eval_chunk_count(),
            "gram_read_gb": round(gram_read / 1e9, 3), "loop_read_gb": round(loop_read / 1e9, 3),
            "gram_tb_s": round(gram_read / med["gram"] / 1e6, 3),
            "loop_tb_s": round(loop_read / med["loop"] / 1e6, 3),
            "gram_partial_tb_s": round(gram_read / max(med["gram"] - med["mult_p"], 1e-9) / 1e6, 3),
            "loop_partial_tb_s": round(loop_read / max(med["loop"] - P * med["dot_k1"], 1e-9) / 1e6, 3),
            "tail_saving_us": round(saving, 2),
            "bound_us": round(med["loop"] - 0.8 * saving, 2),
            "within_bound": bool(med["gram"] <= med["loop"] - 0.8 * saving),
            "loop_over_gram": round(med["loop"] / med["gram"], 3),
        })
        res["shapes"]["C%d_K%d" % (n, K)] = r
        del G, Gl, prod
    print(json.dumps(res))


if __name__ == "__main__":
    main()
