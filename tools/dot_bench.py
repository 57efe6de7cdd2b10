#!/usr/bin/env python3
"""Time D.dot against the per-ciphertext path to the same single ciphertext, in one process.

Shape: ring 2^15, 4 towers, K = 714 ciphertexts (one cfg3 learner) and K = 16.  For each K, alternating inside
every round so drift hits them alike:

  dot_uv    D.dot(u, v)                       algorithmic traffic 4 K towers N 8 bytes
  dot_uu    D.dot(u, u)                       2 K towers N 8 bytes
  parent    D.mult(u, v) over the K pairs, then a halving tree of batched D.add down to one ciphertext
  add       D.add(u, v) over the K pairs      3 K 2 towers N 8 bytes: the streaming rate dot is read against
  dot_k1    D.dot on one pair: the reduction and the K = 1 key switch, i.e. the tail every dot ends in

then the SHELFI_DOT_SLICE_CTS sweep behind the default (the switch is re-read between settings, never on a
launch path).  Each call ends in the library's own stream synchronise, so a host clock around it is a device
time plus one launch chain.  Prints one JSON line: microseconds per call, median and [min, max] over the
rounds, and the bandwidths the medians amount to.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-fed_amd"))

SWITCH = "SHELFI_DOT_SLICE_CTS"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--cts", type=int, nargs="+", default=[714, 16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="calls per round")
    ap.add_argument("--sweep", type=int, nargs="*", default=[1, 2, 4, 8, 16, 64, 128, 256, 1024],
                    help="SHELFI_DOT_SLICE_CTS settings (those giving a slice count already timed at a K are skipped)")
    a = ap.parse_args()

    import torch

    import SHELFI_FHE as m
    from SHELFI_FHE import device as D

    if not torch.cuda.is_available():
        sys.exit("dot_bench needs a GPU: there is no CPU timing to report")
    c = m.CKKS("ckks", a.batch, 52, "", multDepth=a.depth, seed=7, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    c.evalMultKeyGen()
    inf = c.info()
    S, L, N = inf["batch"], inf["num_towers"], inf["ring_dim"]
    Kmax = max(a.cts)
    u = D.encrypt(c, torch.rand(Kmax * S, dtype=torch.float64, device="cuda") * 2 - 1)
    v = D.encrypt(c, torch.rand(Kmax * S, dtype=torch.float64, device="cuda") * 2 - 1)
    prod, tmp = torch.empty_like(u), torch.empty_like(u)
    one = torch.empty((1, 2, L, N), dtype=torch.int64, device="cuda")

    def timed(f, reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps * 1e6

    def parent(K):
        D.mult(c, u[:K], v[:K], out=prod[:K])
        n = K
        while n > 1:  # prod[:h] += prod[n - h:n]; an odd middle ciphertext waits for the next level
            h = n // 2
            D.add(c, prod[:h], prod[n - h:n], out=prod[:h])
            n -= h

    def stat(vals):
        return {"median": round(statistics.median(vals), 2), "min": round(min(vals), 2), "max": round(max(vals), 2)}

    def rounds(ops):
        for f in ops.values():  # warm-up: code objects, level tables, scratch
            f()
            f()
        us = {k: [] for k in ops}
        for _ in range(a.rounds):
            for k, f in ops.items():
                us[k].append(timed(f, a.reps))
        return us

    os.environ.pop(SWITCH, None)
    m.reload_switches()
    res = {"ring_dim": N, "towers": L, "rounds": a.rounds, "reps": a.reps, "by_cts": {}, "sweep": {}}
    poly_bytes = L * N * 8
    for K in a.cts:
        ops = {
            "dot_uv": lambda K=K: D.dot(c, u[:K], v[:K], out=one),
            "dot_uu": lambda K=K: D.dot(c, u[:K], u[:K], out=one),
            "parent": lambda K=K: parent(K),
            "add": lambda K=K: D.add(c, u[:K], v[:K], out=tmp[:K]),
            "dot_k1": lambda: D.dot(c, u[:1], v[:1], out=one),
        }
        us = rounds(ops)
        r = {k + "_us": stat(w) for k, w in us.items()}
        med = {k: statistics.median(w) for k, w in us.items()}
        ops["dot_uv"]()
        r["slices"] = c.dot_slice_count()
        r["dot_uv_tb_s"] = round(4 * K * poly_bytes / med["dot_uv"] / 1e6, 3)
        r["dot_uu_tb_s"] = round(2 * K * poly_bytes / med["dot_uu"] / 1e6, 3)
        r["add_tb_s"] = round(3 * K * 2 * poly_bytes / med["add"] / 1e6, 3)
        r["parent_over_dot_uv"] = round(med["parent"] / med["dot_uv"], 2)
        res["by_cts"][str(K)] = r
        # the sweep: one setting per distinct slice count at this K, alternating inside every round
        seen, ops = set(), {}
        for cts in a.sweep:
            sl = min(16, -(-K // cts))
            if sl in seen:
                continue
            seen.add(sl)

            def run(cts=cts, K=K, sq=False):
                os.environ[SWITCH] = str(cts)
                m.reload_switches()
                D.dot(c, u[:K], u[:K] if sq else v[:K], out=one)

            ops["uv_cts%d_S%d" % (cts, sl)] = run
            ops["uu_cts%d_S%d" % (cts, sl)] = lambda run=run: run(sq=True)
        res["sweep"][str(K)] = {k: stat(w) for k, w in rounds(ops).items()}
        os.environ.pop(SWITCH, None)
        m.reload_switches()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
