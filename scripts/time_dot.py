#!/usr/bin/env python3
"""MI355X timing of the sums of products next to K multiplies: dot_device on K seeded operand pairs
against K calls of mul_device on the same operands (the multiply's code is the parent's: this
feature adds entries and kernels beside it), at C3 and C2 for K = 2 and K = 4, at the dot's size
for both routes.  Each route is warmed up once, then 20 calls on one stream between HIP events, the
two alternating for three rounds each; reports the median and the spread (max - min) of the rounds.
First the sum is checked for equality with the K products added on the host.  Five profiled calls
of each route give the per-stage times, per call (profile_begin / profile_end; a sum claims a call
slot per term, its forward and pointwise times are sums over the terms) -- one call's stage times
scatter by the 1-2 % of a run, which is the size of the second bar's margin.
Asserted: ratio <= (K (F + P) + I) / (K (F + P + I)) + 0.03 with F, P, I the multiply's profiled
forward, pointwise and inverse-side times of the same run, and the k_pwsa stage per term (the
sum's pointwise time less one k_pwss stage, over K - 1) <= 1.05 x the k_pwss stage.
usage: python scripts/time_dot.py [out.json]"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, ROUNDS, PROF_CALLS = 20, 3, 5
FWD, INV = ("fwd_columns", "fwd_rows"), ("inv_rows", "inv_columns", "scale", "combine")


def timed(fn, torch, stream, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def profiled(mp, fn, slots, torch):
    """per-call stage times, the mean of PROF_CALLS calls that claim `slots` call slots each"""
    mp.profile_begin(PROF_CALLS * slots)
    for _ in range(PROF_CALLS):
        fn()
    torch.cuda.synchronize()
    ms, calls = mp.profile_end()
    assert calls == PROF_CALLS * slots, (calls, slots)
    return {k: v / PROF_CALLS for k, v in ms.items()}


def stats(t):
    return {"median": statistics.median(t), "spread": max(t) - min(t), "rounds": t}


def to_int(t):
    return int.from_bytes(t.cpu().numpy().tobytes(), "little")


def main():
    import torch
    import mpfft_loader
    mp = mpfft_loader.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    rows = []
    for name, depth, w, n0 in (("C3", 15, 4, 20312500), ("C2", 15, 4, 15625000)):
        for K in (2, 4):
            n = min(n0, mp.dot_max_limbs(K, depth, w))
            das = [torch.from_numpy(mp.fill_random(n, 0x1001 + i).view(np.int64)).to(dev) for i in range(K)]
            dbs = [torch.from_numpy(mp.fill_random(n, 0x2002 + i).view(np.int64)).to(dev) for i in range(K)]
            dms = [torch.zeros(2 * n, dtype=torch.int64, device=dev) for _ in range(K)]
            dd = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev)
            wsm = mp.alloc_workspace(n, n, depth, w, dev)
            wsd = mp.alloc_workspace_dot(K, n, n, depth, w, dev)

            def muls():
                for i in range(K):
                    mp.mul_device(dms[i], das[i], n, dbs[i], n, depth, w, wsm, stream=stream)
            one_mul = lambda: mp.mul_device(dms[0], das[0], n, dbs[0], n, depth, w, wsm, stream=stream)
            dot = lambda: mp.dot_device(dd, das, dbs, n, n, depth, w, wsd, stream=stream)
            with torch.cuda.stream(stream):
                muls()
                dot()
                torch.cuda.synchronize()
                same = to_int(dd) == sum(to_int(m) for m in dms)
                tm, td = [], []
                for _ in range(ROUNDS):
                    tm.append(timed(muls, torch, stream))
                    td.append(timed(dot, torch, stream))
                sm = profiled(mp, one_mul, 1, torch)
                sd = profiled(mp, dot, K, torch)
            F, P, I = sum(sm[k] for k in FWD), sm["pointwise"], sum(sm[k] for k in INV)
            row = {"name": name, "depth": depth, "w": w, "n": n, "K": K, "same_sum": same,
                   "kernels": mp.dot_stage_kernels(K, n, n, depth, w),
                   "bits1": {"dot": mp.dot_plan_info(K, n, n, depth, w)["bits1"], "mul": mp.plan_info(n, n, depth, w)["bits1"]},
                   "workspace_bytes": {"mul": mp.workspace_bytes(n, n, depth, w), "dot": mp.dot_workspace_bytes(K, n, n, depth, w)},
                   "muls_ms": stats(tm), "dot_ms": stats(td), "stages_ms": {"mul": sm, "dot": sd},
                   "F": F, "P": P, "I": I}
            row["ratio"] = row["dot_ms"]["median"] / row["muls_ms"]["median"]
            row["predicted"] = (K * (F + P) + I) / (K * (F + P + I))
            row["bar"] = row["predicted"] + 0.03
            row["pwsa_per_term_ms"] = (sd["pointwise"] - P) / (K - 1)
            row["pwsa_over_pwss"] = row["pwsa_per_term_ms"] / P
            rows.append(row)
            print(json.dumps(row), flush=True)
            assert same, "dot_device differs from the K products added on the host at %s K = %d" % (name, K)
            del das, dbs, dms, dd, wsm, wsd
            torch.cuda.empty_cache()
    out = sys.argv[1] if len(sys.argv) > 1 else None
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
    late = ["%s K=%d: %.3f > %.3f" % (r["name"], r["K"], r["ratio"], r["bar"]) for r in rows if r["ratio"] > r["bar"]]
    assert not late, "the sum is slower than its bar against K multiplies: " + "; ".join(late)
    slow = ["%s K=%d: %.3f" % (r["name"], r["K"], r["pwsa_over_pwss"]) for r in rows if r["pwsa_over_pwss"] > 1.05]
    assert not slow, "k_pwsa's stage per term above 1.05 x k_pwss's: " + "; ".join(slow)


if __name__ == "__main__":
    main()
