#!/usr/bin/env python3
"""Time D.eval_poly against the composition from existing calls it replaces, in one process.

Shape: ring 2^15, 8 towers (ringDim override); K = 64 and K = 714 ciphertexts; degrees 3, 7 and 15.  For each shape
and degree, alternating inside every round so drift hits them alike:

  eval_poly  D.eval_poly: the powers (one key switch each), ONE combine, 1 or 2 rescales
  powers     its first part alone (D.poly_powers)
  combine    its second part alone (D.poly_combine on those powers)
  rescales   its last part alone
  hand       the composition: x^n = x^ceil(n/2) x^floor(n/2) by D.mult on prefix copies + D.rescale for every
             n = 2..d (d - 1 key switches), the constants by D.encode, every term by D.mult_plain on a prefix copy
             at the lowest level and D.add, one D.rescale, a_0 by D.add_plain
  mult_k     D.mult over K pairs at the combine level: the batched key switch's share of the combine
  add_k      D.add over two batches of K ciphertexts at the combine level: the streaming yardstick, 3 K moved

Each call ends in the library's own stream synchronise (add_k and the prefix copies in torch's), so a host clock
around it is a device time plus its launch chains.  Prints one JSON line: microseconds per call, median and
[min, max] over the rounds; the bytes the combine's front pass reads and writes over the combine's time less
mult_k's (its achieved rate) beside add_k's; hand over eval_poly; and whether eval_poly beats the composition by
more than the rounds' own spread.  Nothing is tuned per shape.
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
    ap.add_argument("--ring", type=int, default=1 << 15)
    ap.add_argument("--depth", type=int, default=7)
    ap.add_argument("--cts", type=int, nargs="+", default=[64, 714])
    ap.add_argument("--degrees", type=int, nargs="+", default=[3, 7, 15])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1, help="calls per round")
    a = ap.parse_args()

    import numpy as np
    import torch

    import SHELFI_FHE as m
    from SHELFI_FHE import device as D

    if not torch.cuda.is_available():
        sys.exit("eval_poly_bench needs a GPU: there is no CPU timing to report")
    c = m.CKKS("ckks", a.ring // 2, 52, "", multDepth=a.depth, ringDim=a.ring, seed=7, decodeNoise=False)
    assert c.genCryptoContextAndKeyGen() == 1
    c.evalMultKeyGen()
    inf = c.info()
    S, L, N, delta = inf["batch"], inf["num_towers"], inf["ring_dim"], inf["delta"]
    rng = np.random.default_rng(7)

    def timed(f, reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps * 1e6

    def stat(vals):
        return {"median": round(statistics.median(vals), 2), "min": round(min(vals), 2), "max": round(max(vals), 2)}

    def prefix(t, towers):
        return t if t.shape[2] == towers else t[:, :, :towers].contiguous()

    res = {"ring_dim": N, "towers": L, "rounds": a.rounds, "reps": a.reps, "shapes": {}}
    for K in a.cts:
        x = D.encrypt(c, torch.rand(K * S, dtype=torch.float64, device="cuda") * 2 - 1)
        for d in a.degrees:
            coeffs = rng.uniform(-1, 1, d + 1)
            pl = D._poly_plan(c, coeffs, L, delta)
            tc, nb, ng = pl["combine_towers"], pl["babies"], pl["giants"] - 1
            have = D.poly_powers(c, x, delta, d)
            babies = [have[j][0] for j in range(1, nb + 1)]
            giants = [have[4 * g][0] for g in range(1, ng + 1)]
            comb = D.poly_combine(c, babies, giants, pl["table"], tc)
            ones = torch.ones(S, dtype=torch.float64, device="cuda")
            ma, mb = prefix(x, tc), prefix(babies[-1], tc)
            tmp = torch.empty_like(ma)

            def rescales():
                o = comb
                for _ in range(pl["rescales"]):
                    o = D.rescale(c, o)
                return o

            def hand():
                pw = {1: x}
                for n in range(2, d + 1):
                    u, v = pw[(n + 1) // 2], pw[n // 2]
                    t = min(u.shape[2], v.shape[2])
                    pw[n] = D.rescale(c, D.mult(c, prefix(u, t), prefix(v, t)))
                t = min(v.shape[2] for v in pw.values())
                acc = None
                for n in range(1, d + 1):
                    pt = D.encode(c, ones * float(coeffs[n]), towers=t, scale=delta)
                    term = D.mult_plain(c, prefix(pw[n], t), pt)
                    acc = term if acc is None else D.add(c, acc, term, out=acc)
                acc = D.rescale(c, acc)  # (a_0 goes in after the rescale: encode takes no scale of delta^2)
                return D.add_plain(c, acc, D.encode(c, ones * float(coeffs[0]), towers=t - 1, scale=delta), out=acc)

            ops = {
                "eval_poly": lambda: D.eval_poly(c, x, coeffs, delta),
                "powers": lambda: D.poly_powers(c, x, delta, d),
                "combine": lambda: D.poly_combine(c, babies, giants, pl["table"], tc, out=comb),
                "rescales": rescales,
                "hand": hand,
                "mult_k": lambda: D.mult(c, ma, mb, out=tmp),
                "add_k": lambda: D.add(c, ma, mb, out=tmp),
            }
            for f in ops.values():  # warm-up: code objects, level tables, scratch, the allocator's pools
                f()
                f()
            us_ = {k: [] for k in ops}
            for _ in range(a.rounds):
                for k, f in ops.items():
                    us_[k].append(timed(f, a.reps))
            r = {k + "_us": stat(w) for k, w in us_.items()}
            med = {k: statistics.median(w) for k, w in us_.items()}
            poly_bytes = tc * N * 8
            # the combine's front pass: both polynomials of every power over the combine level's towers, d0 and d1
            # written to the output, d2 twice to the key switch's scratch (nothing without giants)
            front = K * poly_bytes * (2 * (nb + ng) + 2 + (2 if ng else 0))
            add_rate = 3 * K * 2 * poly_bytes / med["add_k"]  # bytes per microsecond
            r.update({
                "key_switches_eval_poly": len(pl["powers"]) - 1 + (1 if ng else 0), "key_switches_hand": d - 1,
                "combine_towers": tc, "result_towers": pl["result_towers"], "chains": c.eval_chunk_count(),
                "add_tb_s": round(add_rate / 1e6, 3),
                "combine_front_gb": round(front / 1e9, 3),
                "combine_front_tb_s": round(front / max(med["combine"] - (med["mult_k"] if ng else 0), 1e-9) / 1e6, 3),
                "hand_over_eval_poly": round(med["hand"] / med["eval_poly"], 2),
                "faster_beyond_spread": bool(max(us_["eval_poly"]) < min(us_["hand"])),
            })
            res["shapes"]["K%d_d%d" % (K, d)] = r
            del have, babies, giants, comb, ma, mb, tmp
        del x
    print(json.dumps(res))


if __name__ == "__main__":
    main()
