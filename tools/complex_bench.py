#!/usr/bin/env python3
"""Real against complex slot packing in one process.

Shape: ring 2^15, 4 towers, n = 714 * 16384 values -- one cfg3 learner: 714 ciphertexts with one value a
slot, 357 with two.  Measured in both modes, alternating inside every round so drift hits them alike:

  encrypt    device.encrypt of the n values
  arena      Arena.wavg of 16 learners' resident batches (the packed layout)
  decrypt    device.decrypt of the aggregate (decode noise off in both modes: complex slots cannot flood)
  bytes      the bytes-API computeWeightedAverage of 16 learners x the ciphertexts of 64 * 16384 values, in
             the packed wire format (64 / 32 ciphertexts a learner)

and device.conj beside device.rotate on the complex mode's ciphertexts.  Halving the ciphertexts of a call
also halves what its fixed costs are spread over, so encrypt and decrypt are measured a third time: real
mode on n / 2 values ("real_same_cts"), the complex call's ciphertext count, which is the baseline a
per-ciphertext cost is read against.  Every device call ends in the
library's own stream synchronise, so a host clock around it is a device time plus one launch chain.  Every
shape is warmed up first.

--real-only measures real mode alone and calls nothing an older library lacks: with SHELFI_LIB_AB naming
another build (the parent commit's, as tools/lib_ab.sh takes it) the same four measurements run on that
library, for the same-box comparison of real mode with it.

Prints one JSON line: microseconds per ciphertext and values per second, median and [min, max] over the
rounds, and the complex / real ratios of the medians.
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
    ap.add_argument("--cts", type=int, default=714, help="real-mode ciphertexts of the device measurements (even)")
    ap.add_argument("--bytes-cts", type=int, default=64, help="real-mode ciphertexts a learner of the bytes API (even)")
    ap.add_argument("--learners", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3, help="calls per round of the device measurements")
    ap.add_argument("--real-only", action="store_true", help="real mode alone (runs on a library without the mode)")
    a = ap.parse_args()
    if a.cts % 2 or a.bytes_cts % 2:
        sys.exit("the ciphertext counts must be even: complex packing halves them")

    import torch

    import SHELFI_FHE as m
    from SHELFI_FHE import device as D

    if not torch.cuda.is_available():
        sys.exit("complex_bench needs a GPU: there is no CPU timing to report")
    c = m.CKKS("ckks", a.batch, 52, "", multDepth=a.depth, seed=7, decodeNoise=False, wireFormat="packed")
    assert c.genCryptoContextAndKeyGen() == 1
    if not a.real_only:
        c.rotationKeyGen([1])
        c.conjugateKeyGen()
    inf = c.info()
    S, C = inf["batch"], a.learners
    n, nb = a.cts * S, a.bytes_cts * S
    w = [1.0 / C] * C
    x = torch.rand(n, dtype=torch.float64, device="cuda") * 2 - 1
    xb = (torch.rand(nb, dtype=torch.float64) * 2 - 1).numpy()
    scale2 = inf["delta"] * inf["delta"]

    def timed(f, reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps

    # per mode: the ciphertext counts, the resident arena, the aggregate, the learners' blobs
    modes = {}
    for mode in ("real",) if a.real_only else ("real", "complex"):
        if not a.real_only:
            c.set_slot_packing(mode)
        V = c.info()["values_per_ct"]
        K, Kb = n // V, nb // V
        ct = D.encrypt(c, x)
        assert ct.shape[0] == K
        arena = D.Arena(c, C, K)
        for i in range(C):
            arena.put(i, ct)
        agg = arena.wavg(w)
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        blobs = [c.encrypt(xb)] * C
        modes[mode] = dict(K=K, Kb=Kb, ct=ct, arena=arena, agg=agg, out=out, blobs=blobs, enc=torch.empty_like(ct))

    # real mode at the complex call's ciphertext count: n / 2 values
    Kh = a.cts // 2
    xh = x[:Kh * S]
    if not a.real_only:
        c.set_slot_packing("real")
        modes["real_same_cts"] = dict(K=Kh, enc=torch.empty_like(modes["complex"]["ct"]), agg=modes["real"]["agg"][:Kh],
                                      out=torch.empty(Kh * S, dtype=torch.float64, device="cuda"))

    def ops(mode):
        s = modes[mode]
        if mode == "real_same_cts":
            return {
                "encrypt": (lambda: D.encrypt(c, xh, out=s["enc"]), a.reps, s["K"], Kh * S),
                "decrypt": (lambda: D.decrypt(c, s["agg"], Kh * S, scale2, out=s["out"]), a.reps, s["K"], Kh * S),
            }
        return {
            "encrypt": (lambda: D.encrypt(c, x, out=s["enc"]), a.reps, s["K"], n),
            "arena": (lambda: s["arena"].wavg(w, out=s["agg"]), a.reps, s["K"], n),
            "decrypt": (lambda: D.decrypt(c, s["agg"], n, scale2, out=s["out"]), a.reps, s["K"], n),
            "bytes": (lambda: c.computeWeightedAverage(s["blobs"], w), 1, C * s["Kb"], C * nb),
        }

    def packing(mode):
        return "complex" if mode == "complex" else "real"

    sec = {mode: {k: [] for k in ops(mode)} for mode in modes}
    def set_mode(mode):
        if not a.real_only:
            c.set_slot_packing(packing(mode))

    for mode in modes:  # warm-up: code objects, scratch, the staging ring
        set_mode(mode)
        for f, _, _, _ in ops(mode).values():
            f()
            f()
    for _ in range(a.rounds):
        for mode in modes:
            set_mode(mode)
            for k, (f, reps, _, _) in ops(mode).items():
                sec[mode][k].append(timed(f, reps))

    def stat(v, digits):
        return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}

    res = {"ring_dim": inf["ring_dim"], "towers": inf["num_towers"], "batch": S, "values": n, "bytes_values": nb,
           "learners": C, "rounds": a.rounds}
    for mode in modes:
        o = ops(mode)
        res[mode] = {"cts": modes[mode]["K"]}
        if "Kb" in modes[mode]:
            res[mode]["bytes_cts_per_learner"] = modes[mode]["Kb"]
        for k, v in sec[mode].items():
            cts, vals = o[k][2], o[k][3]
            res[mode][k] = {"us_per_ct": stat([t / cts * 1e6 for t in v], 3),
                            "values_per_s": stat([vals / t for t in v], 0)}
    if a.real_only:
        res["library"] = os.environ.get("SHELFI_LIB_AB", "in-tree")
        print(json.dumps(res))
        return
    res["complex_over_real"] = {}
    for k in sec["real"]:
        r, z = statistics.median(sec["real"][k]), statistics.median(sec["complex"][k])
        kr, kz = ops("real")[k][2], ops("complex")[k][2]
        res["complex_over_real"][k] = {"us_per_ct": round((z / kz) / (r / kr), 4), "values_per_s": round(r / z, 4)}
    res["complex_over_real_same_cts"] = {
        k: {"us_per_ct": round(statistics.median(sec["complex"][k]) / statistics.median(v), 4)}
        for k, v in sec["real_same_cts"].items()}

    # conj beside rotate, on the complex mode's ciphertexts
    c.set_slot_packing("complex")
    ct, K = modes["complex"]["ct"], modes["complex"]["K"]
    out = torch.empty_like(ct)
    gal = {"rotate": lambda: D.rotate(c, ct, 1, out=out), "conj": lambda: D.conj(c, ct, out=out)}
    for f in gal.values():
        f()
        f()
    us = {k: [] for k in gal}
    for _ in range(a.rounds):
        for k, f in gal.items():
            us[k].append(timed(f, a.reps) / K * 1e6)
    for k, v in us.items():
        res[k + "_us_per_ct"] = stat(v, 3)
    res["conj_over_rotate"] = round(statistics.median(us["conj"]) / statistics.median(us["rotate"]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
