#!/usr/bin/env python3
"""MI355X timing of the squaring entry next to the multiply of an operand by itself:
sqr_device(a) and mul_device(a, a) on the same seeded operand, each warmed up once, then 20
calls on one stream between HIP events, the two alternating for three rounds each; reports the
median and the spread (max - min) of the rounds and asserts that the two products are equal.
At C3 one profiled call of each also gives the per-stage times (profile_begin / profile_end).
usage: python scripts/time_sqr.py [out.json]"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, ROUNDS = 20, 3


def timed(fn, torch, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(REPS):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def profiled(mp, fn, torch):
    mp.profile_begin(1)
    fn()
    torch.cuda.synchronize()
    ms, calls = mp.profile_end()
    assert calls == 1
    return ms


def main():
    import torch
    import mpfft_loader
    mp = mpfft_loader.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    rows = []
    cases = [("C3", 15, 4, 20312500), ("C2", 15, 4, 15625000), ("C4", 17, 2, 156250000), ("small", 11, 8, 261952)]
    for name, depth, w, n in cases:
        a = mp.fill_random(n, 0x1001)
        da = torch.from_numpy(a.view(np.int64)).to(dev)
        del a
        dm = torch.zeros(2 * n, dtype=torch.int64, device=dev)
        ds = torch.zeros(2 * n, dtype=torch.int64, device=dev)
        wsm = mp.alloc_workspace(n, n, depth, w, dev)
        wss = mp.alloc_workspace_sqr(n, depth, w, dev)
        mul = lambda: mp.mul_device(dm, da, n, da, n, depth, w, wsm, stream=stream)
        sqr = lambda: mp.sqr_device(ds, da, n, depth, w, wss, stream=stream)
        with torch.cuda.stream(stream):
            mul()
            sqr()
            torch.cuda.synchronize()
            same = bool(torch.equal(dm, ds))
            tm, ts = [], []
            for _ in range(ROUNDS):
                tm.append(timed(mul, torch, stream))
                ts.append(timed(sqr, torch, stream))
            row = {"name": name, "depth": depth, "w": w, "n": n, "same_product": same,
                   "pointwise": {"mul": mp.stage_kernels(n, n, depth, w)["pointwise"],
                                 "sqr": mp.sqr_stage_kernels(n, depth, w)["pointwise"]},
                   "workspace_bytes": {"mul": mp.workspace_bytes(n, n, depth, w), "sqr": mp.sqr_workspace_bytes(n, depth, w)},
                   "mul_ms": {"median": statistics.median(tm), "spread": max(tm) - min(tm), "rounds": tm},
                   "sqr_ms": {"median": statistics.median(ts), "spread": max(ts) - min(ts), "rounds": ts}}
            row["ratio"] = row["sqr_ms"]["median"] / row["mul_ms"]["median"]
            if name == "C3":
                row["stages_ms"] = {"mul": profiled(mp, mul, torch), "sqr": profiled(mp, sqr, torch)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        assert same, "sqr_device(a) differs from mul_device(a, a) at %s" % name
        del wsm, wss, dm, ds, da
        torch.cuda.empty_cache()
    out = sys.argv[1] if len(sys.argv) > 1 else None
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
    # acceptance: the halved forward stages alone make a square at most 0.90 x the multiply at C3, C2
    late = [r["name"] for r in rows if r["name"] in ("C3", "C2") and r["ratio"] > 0.90]
    assert not late, "square slower than 0.90 x the multiply at " + ", ".join(late)


if __name__ == "__main__":
    main()
