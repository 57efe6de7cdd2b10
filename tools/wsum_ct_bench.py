#!/usr/bin/env python3
"""Time D.wsum_ct against the two compositions it replaces, in one process.

Shape: ring 2^15, 4 towers; C = 16 learners of K = 714 ciphertexts (cfg3) and C = 4 of K = 16.  For each shape,
alternating inside every round so drift hits them alike:

  wsum_kw1  D.wsum_ct with one weight ciphertext a learner     K results, one key switch of K
  wsum_kwk  D.wsum_ct with one weight ciphertext per update ciphertext
  mults     for every learner D.mult(w_c, u_c) over its K ciphertexts (per-ciphertext weights, so nothing has
            to be replicated first), then D.add into the running sum: C K key switches
  dots      for every k the gather of the learners' k-th ciphertexts into one batch (the weights' too: once a
            call with one weight a learner, every k with one per ciphertext), then D.dot: K key switches of one
            ciphertext each, the gathers counted
  mult_k    D.mult over K ciphertext pairs: the batched key switch's share of wsum_ct
  add_k     D.add over two batches of K ciphertexts: the streaming yardstick, 3 K ciphertexts moved

Each call ends in the library's own stream synchronise (add_k in torch's), so a host clock around it is a device
time plus its launch chains.  Prints one JSON line: microseconds per call, median and [min, max] over the rounds;
the bytes wsum_ct's front pass reads and writes over the call's time less mult_k's (its achieved rate) beside
add_k's; the expectation mult_k + input bytes / add_k's rate; and whether wsum_ct beats both compositions by
more than the rounds' own spread.
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
    ap.add_argument("--shapes", type=int, nargs="+", default=[16, 714, 4, 16], help="C K [C K ...]")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=2, help="calls per round")
    a = ap.parse_args()

    import torch

    import SHELFI_FHE as m
    from SHELFI_FHE import device as D

    if not torch.cuda.is_available():
        sys.exit("wsum_ct_bench needs a GPU: there is no CPU timing to report")
    c = m.CKKS("ckks", a.batch, 52, "", multDepth=a.depth, seed=7, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    c.evalMultKeyGen()
    inf = c.info()
    S, L, N = inf["batch"], inf["num_towers"], inf["ring_dim"]
    shapes = list(zip(a.shapes[0::2], a.shapes[1::2]))
    Cmax, Kmax = max(s[0] for s in shapes), max(s[1] for s in shapes)

    def fresh(lo):
        return D.encrypt(c, torch.rand(Kmax * S, dtype=torch.float64, device="cuda") * (1 - lo) + lo)

    us = [fresh(-1) for _ in range(Cmax)]
    ws = [fresh(0) for _ in range(Cmax)]

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
        bu, bw = [u[:K] for u in us[:n]], [w[:K] for w in ws[:n]]
        b1 = [w[:1] for w in ws[:n]]
        o1, ok, om, od1, odk, tmp = (torch.empty((K, 2, L, N), dtype=torch.int64, device="cuda") for _ in range(6))
        gu, gw = (torch.empty((n, 2, L, N), dtype=torch.int64, device="cuda") for _ in range(2))

        def mults():
            D.mult(c, bw[0], bu[0], out=om)
            for i in range(1, n):
                D.mult(c, bw[i], bu[i], out=tmp)
                D.add(c, om, tmp, out=om)

        def dots(per_k, out):
            if not per_k:
                torch.stack([w[0] for w in b1], out=gw)
            for k in range(K):
                torch.stack([u[k] for u in bu], out=gu)
                if per_k:
                    torch.stack([w[k] for w in bw], out=gw)
                D.dot(c, gw, gu, out=out[k:k + 1])

        ops = {
            "wsum_kw1": lambda: D.wsum_ct(c, bu, b1, out=o1),
            "wsum_kwk": lambda: D.wsum_ct(c, bu, bw, out=ok),
            "mults": mults,
            "dots_kw1": lambda: dots(False, od1),
            "dots_kwk": lambda: dots(True, odk),
            "mult_k": lambda: D.mult(c, bw[0], bu[0], out=tmp),
            "add_k": lambda: D.add(c, bw[0], bu[0], out=tmp),
        }
        for f in ops.values():  # warm-up: code objects, level tables, scratch
            f()
            f()
        assert torch.equal(o1, od1) and torch.equal(ok, odk), "wsum_ct differs from the dots it replaces"
        us_ = {k: [] for k in ops}
        for _ in range(a.rounds):
            for k, f in ops.items():
                us_[k].append(timed(f, a.reps))
        r = {k + "_us": stat(w) for k, w in us_.items()}
        med = {k: statistics.median(w) for k, w in us_.items()}
        lo, hi = {k: min(w) for k, w in us_.items()}, {k: max(w) for k, w in us_.items()}
        ops["wsum_kw1"]()
        add_rate = 3 * K * ct_bytes / med["add_k"]  # bytes per microsecond
        # the front pass: every update once, the weights once (per ciphertext) or from cache, c0 and c1 written to
        # the output, c2 twice to the key switch's scratch
        out_bytes = K * 2 * ct_bytes
        in1, ink = (n * K + n) * ct_bytes, 2 * n * K * ct_bytes
        r.update({
            "chains": c.eval_chunk_count(),
            "add_tb_s": round(add_rate / 1e6, 3),
            "input_gb_kw1": round(in1 / 1e9, 3), "input_gb_kwk": round(ink / 1e9, 3),
            "expected_kw1_us": round(med["mult_k"] + in1 / add_rate, 2),
            "expected_kwk_us": round(med["mult_k"] + ink / add_rate, 2),
            "front_kw1_tb_s": round((in1 + out_bytes) / max(med["wsum_kw1"] - med["mult_k"], 1e-9) / 1e6, 3),
            "front_kwk_tb_s": round((ink + out_bytes) / max(med["wsum_kwk"] - med["mult_k"], 1e-9) / 1e6, 3),
            "mults_over_wsum_kwk": round(med["mults"] / med["wsum_kwk"], 2),
            "dots_over_wsum_kw1": round(med["dots_kw1"] / med["wsum_kw1"], 2),
            "dots_over_wsum_kwk": round(med["dots_kwk"] / med["wsum_kwk"], 2),
            # slower than wsum_ct's slowest round in every round of their own
            "beats_both_beyond_spread": bool(hi["wsum_kwk"] < lo["mults"] and hi["wsum_kwk"] < lo["dots_kwk"]
                                             and hi["wsum_kw1"] < lo["mults"] and hi["wsum_kw1"] < lo["dots_kw1"]),
        })
        res["shapes"]["C%d_K%d" % (n, K)] = r
        del o1, ok, om, od1, odk, tmp, gu, gw
    print(json.dumps(res))


if __name__ == "__main__":
    main()
