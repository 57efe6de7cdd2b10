#!/usr/bin/env python3
"""Time D.dot_plain, D.project and D.pack_slots against the paths they replace, in one process.

Shape: ring 2^15, 4 towers.  The contenders of a shape alternate inside every round so drift hits them alike:

  (a) C = R = 1, K = 714 (one cfg3 learner against one known vector)
      dot_plain    D.dot_plain(u, p)                   algorithmic traffic 3 K towers N 8 bytes
      parent       D.mult_plain(u, p) over the K pairs, then a halving tree of batched D.add down to one ciphertext
      mult_plain   the parent's first pass alone       5 K towers N 8 bytes
      add          D.add(u, v) over the K pairs        6 K towers N 8 bytes: the streaming rate the rest is read against
  (b) C = 16, R = 1, K = 714
      project      D.project(16 learners, p)           (2 C + ceil(C / 4)) K towers N 8 bytes
      loop         16 D.dot_plain calls
  (c) K = 136 ciphertexts of one number each (a Gram matrix of 16 learners after eval_sum)
      pack_open    D.pack_slots, then D.decrypt of the ONE ciphertext
      open_each    D.decrypt of the 136

The compared outputs are checked for equality first.  Two conditions were set before the first run: dot_plain at
(a) takes no longer than the mult_plain pass over the same K alone, and project at (b) no longer than its loop.
A call that sums in one slice returns with its work enqueued; the clock stops behind a device synchronise either
way.  Writes one JSON line to --out and prints it: microseconds per call, median and [min, max] over the rounds,
and the bandwidths the medians amount to.
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
    ap.add_argument("--learners", type=int, default=16)
    ap.add_argument("--numbers", type=int, default=136)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="calls per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dot_plain_bench.json"))
    a = ap.parse_args()

    import torch

    import SHELFI_FHE as m
    from SHELFI_FHE import device as D

    if not torch.cuda.is_available():
        sys.exit("dot_plain_bench needs a GPU: there is no CPU timing to report")
    c = m.CKKS("ckks", a.batch, 52, "", multDepth=a.depth, seed=7, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    S, L, N = inf["batch"], inf["num_towers"], inf["ring_dim"]
    K, C = a.cts, a.learners
    # timing does not depend on the residues: uniform ones below 2^51, canonical in every tower of the chain
    assert min(inf["moduli"]) > 1 << 51
    us = torch.randint(0, 1 << 51, (C, K, 2, L, N), dtype=torch.int64, device="cuda")
    p = torch.randint(0, 1 << 51, (K, L, N), dtype=torch.int64, device="cuda")
    u, v = us[0], us[1]
    prod, tmp = torch.empty_like(u), torch.empty_like(u)
    one = torch.empty((1, 2, L, N), dtype=torch.int64, device="cuda")
    outs = torch.empty((C, 2, L, N), dtype=torch.int64, device="cuda")
    loop = torch.empty_like(outs)

    def timed(f, reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps * 1e6

    def parent():
        D.mult_plain(c, u, p, out=prod)
        n = K
        while n > 1:  # prod[:h] += prod[n - h:n]; an odd middle ciphertext waits for the next level
            h = n // 2
            D.add(c, prod[:h], prod[n - h:n], out=prod[:h])
            n -= h

    def each():
        for i in range(C):
            D.dot_plain(c, us[i], p, out=loop[i:i + 1])

    def stat(vals):
        return {"median": round(statistics.median(vals), 2), "min": round(min(vals), 2), "max": round(max(vals), 2)}

    def rounds(ops):
        for f in ops.values():  # warm-up: code objects, scratch
            f()
            f()
        us_ = {k: [] for k in ops}
        for _ in range(a.rounds):
            for k, f in ops.items():
                us_[k].append(timed(f, a.reps))
        return us_

    res = {"ring_dim": N, "towers": L, "rounds": a.rounds, "reps": a.reps, "cts": K, "learners": C}
    poly_bytes = L * N * 8

    # (a) one learner against one vector
    D.dot_plain(c, u, p, out=one)
    sa = c.dotp_slice_count()
    parent()
    torch.cuda.synchronize()
    assert torch.equal(one, prod[:1]), "dot_plain differs from mult_plain + the tree of adds"
    ops = {
        "dot_plain": lambda: D.dot_plain(c, u, p, out=one),
        "parent": parent,
        "mult_plain": lambda: D.mult_plain(c, u, p, out=prod),
        "add": lambda: D.add(c, u, v, out=tmp),
    }
    w = rounds(ops)
    med = {k: statistics.median(x) for k, x in w.items()}
    r = {k + "_us": stat(x) for k, x in w.items()}
    r["slices"] = sa
    r["dot_plain_tb_s"] = round(3 * K * poly_bytes / med["dot_plain"] / 1e6, 3)
    r["mult_plain_tb_s"] = round(5 * K * poly_bytes / med["mult_plain"] / 1e6, 3)
    r["add_tb_s"] = round(6 * K * poly_bytes / med["add"] / 1e6, 3)
    r["parent_over_dot_plain"] = round(med["parent"] / med["dot_plain"], 2)
    r["condition_1_dot_plain_within_mult_plain"] = bool(med["dot_plain"] <= med["mult_plain"])
    res["a"] = r

    # (b) C learners against one vector
    D.project(c, us, p, out=outs)
    sb = c.dotp_slice_count()
    each()
    torch.cuda.synchronize()
    assert torch.equal(outs, loop), "project differs from its dot_plain loop"
    w = rounds({"project": lambda: D.project(c, us, p, out=outs), "loop": each})
    med = {k: statistics.median(x) for k, x in w.items()}
    r = {k + "_us": stat(x) for k, x in w.items()}
    r["slices"] = sb
    r["project_tb_s"] = round((2 * C + -(-C // 4)) * K * poly_bytes / med["project"] / 1e6, 3)
    r["loop_tb_s"] = round(3 * C * K * poly_bytes / med["loop"] / 1e6, 3)
    r["loop_over_project"] = round(med["loop"] / med["project"], 2)
    r["condition_2_project_within_loop"] = bool(med["project"] <= med["loop"])
    res["b"] = r
    del us, u, v, prod, tmp, loop, outs, p

    # (c) P ciphertexts of one number each, opened by one decrypt or by P
    P = a.numbers
    vals = torch.rand(P, dtype=torch.float64, device="cuda") * 100 - 50
    cts = D.encrypt(c, vals.repeat_interleave(S))
    assert cts.shape == (P, 2, L, N)
    delta = inf["delta"]
    opened = torch.empty(S, dtype=torch.float64, device="cuda")
    every = torch.empty(P * S, dtype=torch.float64, device="cuda")

    def pack_open():
        D.decrypt(c, D.pack_slots(c, cts), S, delta, out=opened)

    def open_each():
        D.decrypt(c, cts, P * S, delta, out=every)

    pack_open()
    open_each()
    torch.cuda.synchronize()
    err = float((opened[:P] - every.view(P, S)[:, 0]).abs().max())
    assert err < 1e-6 and float((opened[:P] - vals).abs().max()) < 1e-6, err
    w = rounds({"pack_open": pack_open, "open_each": open_each,
                "pack_slots": lambda: D.pack_slots(c, cts)})
    med = {k: statistics.median(x) for k, x in w.items()}
    r = {k + "_us": stat(x) for k, x in w.items()}
    r["numbers"] = P
    r["max_difference"] = err
    r["open_each_over_pack_open"] = round(med["open_each"] / med["pack_open"], 2)
    res["c"] = r

    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
