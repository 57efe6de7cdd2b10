#!/usr/bin/env python3
"""Time the plaintext-operand calls beside their yardsticks in one process.

Shape: ring 2^15, 4 towers, K = 714 ciphertexts (one cfg3 learner), device-resident, steady state.
  * D.encode beside D.encrypt: encode does a strict subset of encrypt's work (one of three transforms,
    no sampling, no key combine) behind the same FFT.  Both calls end in the library's own stream
    synchronise, so HIP events around them bracket finished work.
  * D.mult_plain (Kp = K and Kp = 1), D.add_plain, D.sub and D.neg beside D.add, the streaming kernel
    the ciphertext calls already had: microseconds per ciphertext and bytes/s over the algorithmic
    traffic, in units of towers * N * 8 bytes per ciphertext -- add 6 (two ciphertexts in, one out),
    mult_plain 5 (Kp = K: c0, c1 and the plaintext in, c0, c1 out) or 4 (Kp = 1: the one plaintext stays
    in L2), add_plain in place 3 (c0 and the plaintext in, c0 out), sub 6, neg 4.
Every shape is warmed up; the operations alternate inside every round, so drift hits them alike; HIP
events bracket `reps` back-to-back calls.  Prints one JSON line: median and [min, max] over the rounds.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-fed_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--cts", type=int, default=714)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10, help="pointwise calls per round (encode / encrypt: 2)")
    a = ap.parse_args()

    import torch

    import SHELFI_FHE as m
    from SHELFI_FHE import device as D

    if not torch.cuda.is_available():
        sys.exit("plain_ops_probe needs a GPU: there is no CPU timing to report")
    c = m.CKKS("ckks", a.batch, 52, "", multDepth=a.depth, seed=7, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    inf = c.info()
    S, K, L, N = inf["batch"], a.cts, inf["num_towers"], inf["ring_dim"]
    x = torch.rand(K * S, dtype=torch.float64, device="cuda") * 2 - 1
    ct, ct2 = D.encrypt(c, x), D.encrypt(c, x.flip(0))
    pt = D.encode(c, x)
    out, pout = torch.empty_like(ct), torch.empty_like(pt)
    unit = L * N * 8  # bytes of one polynomial over every tower

    def timed(f, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps / K  # us per ciphertext

    # name -> (call, reps, traffic units per ciphertext or None)
    ops = {
        "encrypt": (lambda: D.encrypt(c, x, out=ct2), 2, None),
        "encode": (lambda: D.encode(c, x, out=pout), 2, None),
        "add": (lambda: D.add(c, ct, ct2, out=out), a.reps, 6),
        "mult_plain": (lambda: D.mult_plain(c, ct, pt, out=out), a.reps, 5),
        "mult_plain_kp1": (lambda: D.mult_plain(c, ct, pt[:1], out=out), a.reps, 4),
        "add_plain_inplace": (lambda: D.add_plain(c, out, pt, out=out), a.reps, 3),
        "sub": (lambda: D.sub(c, ct, ct2, out=out), a.reps, 6),
        "neg": (lambda: D.neg(c, ct, out=out), a.reps, 4),
    }
    for f, _, _ in ops.values():  # warm-up: code objects, scratch
        f()
        f()
    us = {k: [] for k in ops}
    for _ in range(a.rounds):
        for k, (f, reps, _) in ops.items():
            us[k].append(timed(f, reps))
    res = {"ring_dim": N, "towers": L, "batch": S, "cts": K, "rounds": a.rounds, "reps": a.reps}
    med = {k: statistics.median(v) for k, v in us.items()}
    for k, v in us.items():
        res[k + "_us_per_ct"] = {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        units = ops[k][2]
        if units:
            res[k + "_GBps"] = round(units * unit / med[k] * 1e-3, 1)
    res["encode_over_encrypt"] = round(med["encode"] / med["encrypt"], 4)
    for k in ("mult_plain", "mult_plain_kp1", "add_plain_inplace", "sub", "neg"):
        res[k + "_GBps_over_add"] = round(res[k + "_GBps"] / res["add_GBps"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
