#!/usr/bin/env python3
"""MI355X timing of the multiply against a precomputed operand next to the plain multiply:
mul_device(a, b) and mul_precomp_device(a, precomp_device(b)) on the same seeded operands, each
warmed up once, then 20 calls on one stream between HIP events, the two alternating for three
rounds each; reports the median and the spread (max - min) of the rounds, the cost of one
precomp_device call (five calls between events, three rounds), the break-even number of multiplies
per precomputation, and asserts that the two products are equal.  At C3 and C4 five profiled calls
of each (and of the precomputation) give the per-stage times (profile_begin / profile_end).
usage: python scripts/time_precomp.py [out.json]"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, ROUNDS, PRE_REPS, PROF_CALLS = 20, 3, 5, 5


def timed(fn, torch, stream, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def profiled(mp, fn, torch):
    """per-call stage times, the mean of PROF_CALLS profiled calls"""
    mp.profile_begin(PROF_CALLS)
    for _ in range(PROF_CALLS):
        fn()
    torch.cuda.synchronize()
    ms, calls = mp.profile_end()
    assert calls == PROF_CALLS
    return {k: v / calls for k, v in ms.items()}


def stats(t):
    return {"median": statistics.median(t), "spread": max(t) - min(t), "rounds": t}


def main():
    import torch
    import mpfft_loader
    mp = mpfft_loader.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    rows = []
    cases = [("C3", 15, 4, 20312500), ("C2", 15, 4, 15625000), ("C4", 17, 2, 156250000), ("small", 11, 8, 261952)]
    for name, depth, w, n in cases:
        a, b = mp.fill_random(n, 0x1001), mp.fill_random(n, 0x2002)
        da = torch.from_numpy(a.view(np.int64)).to(dev)
        db = torch.from_numpy(b.view(np.int64)).to(dev)
        del a, b
        dm = torch.zeros(2 * n, dtype=torch.int64, device=dev)
        dp = torch.zeros(2 * n, dtype=torch.int64, device=dev)
        wsm = mp.alloc_workspace(n, n, depth, w, dev)
        wsp = mp.alloc_workspace_mul_precomp(n, n, depth, w, dev)
        pre = mp.alloc_precomp(n, n, depth, w, dev)
        mul = lambda: mp.mul_device(dm, da, n, db, n, depth, w, wsm, stream=stream)
        mkp = lambda: mp.precomp_device(pre, db, n, n, depth, w, wsm, stream=stream)
        mulp = lambda: mp.mul_precomp_device(dp, da, n, pre, n, depth, w, wsp, stream=stream)
        with torch.cuda.stream(stream):
            mkp()
            mul()
            mulp()
            torch.cuda.synchronize()
            same = bool(torch.equal(dm, dp))
            tm, tp = [], []
            for _ in range(ROUNDS):
                tm.append(timed(mul, torch, stream))
                tp.append(timed(mulp, torch, stream))
            tk = [timed(mkp, torch, stream, PRE_REPS) for _ in range(ROUNDS)]
            row = {"name": name, "depth": depth, "w": w, "n": n, "same_product": same,
                   "kernels": mp.precomp_stage_kernels(n, n, depth, w),
                   "pointwise_mul": mp.stage_kernels(n, n, depth, w)["pointwise"],
                   "precomp_bytes": mp.precomp_bytes(n, n, depth, w),
                   "workspace_bytes": {"mul": mp.workspace_bytes(n, n, depth, w),
                                       "mul_precomp": mp.mul_precomp_workspace_bytes(n, n, depth, w)},
                   "mul_ms": stats(tm), "mul_precomp_ms": stats(tp), "precomp_ms": stats(tk)}
            row["ratio"] = row["mul_precomp_ms"]["median"] / row["mul_ms"]["median"]
            saved = row["mul_ms"]["median"] - row["mul_precomp_ms"]["median"]
            row["break_even_multiplies"] = row["precomp_ms"]["median"] / saved if saved > 0 else None
            if name in ("C3", "C4"):
                row["stages_ms"] = {"mul": profiled(mp, mul, torch), "mul_precomp": profiled(mp, mulp, torch),
                                    "precomp": profiled(mp, mkp, torch)}
                torch.cuda.synchronize()
                same = same and bool(torch.equal(dm, dp))
        rows.append(row)
        print(json.dumps(row), flush=True)
        assert same, "mul_precomp_device(a, pre) differs from mul_device(a, b) at %s" % name
        del wsm, wsp, pre, dm, dp, da, db
        torch.cuda.empty_cache()
    out = sys.argv[1] if len(sys.argv) > 1 else None
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
    # acceptance.  Whole multiply: operand B's outer forward stages alone are 1.0 of 7.28 ms at C3
    # (DESIGN section 9), 0.86; at most 0.90 at C3 and C2 with 0.04 for noise and the larger B read
    late = [r["name"] for r in rows if r["name"] in ("C3", "C2") and r["ratio"] > 0.90]
    assert not late, "multiply against the cache slower than 0.90 x the multiply at " + ", ".join(late)
    # pointwise stage: k_pwsp below k_pwss on the same shape in the same run, at C3 and C4
    slow = [r["name"] for r in rows if "stages_ms" in r
            and r["stages_ms"]["mul_precomp"]["pointwise"] >= r["stages_ms"]["mul"]["pointwise"]]
    assert not slow, "k_pwsp's stage not below k_pwss's at " + ", ".join(slow)


if __name__ == "__main__":
    main()
