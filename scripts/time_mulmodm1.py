#!/usr/bin/env python3
"""MI355X timing of the products mod 2^B - 1 next to the product mod 2^B + 1 at the same
(L, depth, w) and to the full product: mulmodm1_device(a, b), sqrmodm1_device(a),
mulmodm1_mul_precomp_device(a, cache of b), mulmod_device(a, b) and mul_device(a, b) at
choose(L, L)'s pair.  First the results are checked: mulmodm1 against the full product folded on
the host at 2^B == 1, the cached route and the square limb-equal to mulmodm1.  Each entry is warmed
up once, then 20 calls on one stream between HIP events, the entries alternating for three rounds
each; reports the median and the spread (max - min) of the rounds, the ratios, one profiled call's
per-stage times of each (profile_begin / profile_end), the precomputation's time and its
break-even.
Case: the full-efficiency shape (14, 8), L = 33 550 336 (l = 2048, 32 768 slots).
Bars (margin: the larger of the two spreads): mulmodm1 <= mulmod, cached <= mulmodm1,
sqrmodm1 <= mulmodm1.
usage: python scripts/time_mulmodm1.py [out.json]"""
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


def fold(prod, L):
    """the 2 L-limb product mod 2^(64 L) - 1 as an integer, fully reduced"""
    v = int.from_bytes(prod.tobytes(), "little")
    B = 64 * L
    mask = (1 << B) - 1
    while v >> B:
        v = (v & mask) + (v >> B)
    return 0 if v == mask else v


def stats(t):
    return {"median": statistics.median(t), "spread": max(t) - min(t), "rounds": t}


def main():
    import torch
    import mpfft_loader
    mp = mpfft_loader.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    L, depth, w = 33550336, 14, 8
    assert mp.mulmodm1_next_size(L) == (L, depth, w)
    md, mw = mp.choose(L, L)
    a, b = mp.fill_random(L + 1, 0x1001), mp.fill_random(L + 1, 0x2002)
    a[L] = b[L] = 0   # the mod 2^B + 1 entry reads L + 1 limbs
    da = torch.from_numpy(a.view(np.int64)).to(dev)
    db = torch.from_numpy(b.view(np.int64)).to(dev)
    del a, b
    dm = torch.zeros(2 * L, dtype=torch.int64, device=dev)
    dp = torch.zeros(L + 1, dtype=torch.int64, device=dev)
    dr, ds, dc, dq = (torch.zeros(L, dtype=torch.int64, device=dev) for _ in range(4))
    wsm = mp.alloc_workspace(L, L, md, mw, dev)
    wsp = mp.alloc_workspace_mulmod(L, depth, w, False, dev)
    wsr = mp.alloc_workspace_mulmodm1(L, depth, w, mp.M1_MUL, dev)
    wss = mp.alloc_workspace_mulmodm1(L, depth, w, mp.M1_SQR, dev)
    wsc = mp.alloc_workspace_mulmodm1(L, depth, w, mp.M1_PRE, dev)
    pre = mp.alloc_precomp_mulmodm1(L, depth, w, dev)
    entries = {
        "mul": lambda: mp.mul_device(dm, da, L, db, L, md, mw, wsm, stream=stream),
        "mulmod": lambda: mp.mulmod_device(dp, da, db, L, depth, w, wsp, stream=stream),
        "mulmodm1": lambda: mp.mulmodm1_device(dr, da, db, L, depth, w, wsr, stream=stream),
        "sqrmodm1": lambda: mp.sqrmodm1_device(ds, da, L, depth, w, wss, stream=stream),
        "mulmodm1_precomp": lambda: mp.mulmodm1_mul_precomp_device(dc, da, pre, L, depth, w, wsc, stream=stream),
        "precomp": lambda: mp.mulmodm1_precomp_device(pre, db, L, depth, w, wsr, stream=stream),
    }
    with torch.cuda.stream(stream):
        for name in ("precomp", "mul", "mulmod", "mulmodm1", "sqrmodm1", "mulmodm1_precomp"):
            entries[name]()
        mp.mulmodm1_device(dq, da, da, L, depth, w, wsr, stream=stream)
        torch.cuda.synchronize()
        want = fold(dm.cpu().numpy().view(np.uint64), L)
        same = {"mulmodm1 == folded mul": int.from_bytes(dr.cpu().numpy().tobytes(), "little") == want,
                "cached == mulmodm1": bool(torch.equal(dc, dr)),
                "sqrmodm1 == mulmodm1(a, a)": bool(torch.equal(ds, dq))}
        del want, dq
        t = {k: [] for k in entries}
        for _ in range(ROUNDS):
            for k in entries:
                t[k].append(timed(entries[k], torch, stream))
        row = {"L": L, "depth": depth, "w": w, "plan": mp.mulmodm1_plan_info(L, depth, w),
               "mul": {"depth": md, "w": mw, **mp.plan_info(L, L, md, mw)}, "same": same,
               "kernels": {"mulmodm1": mp.mulmodm1_stage_kernels(L, depth, w), "mulmod": mp.mulmod_stage_kernels(L, depth, w),
                           "sqrmodm1": mp.mulmodm1_stage_kernels(L, depth, w, mp.M1_SQR),
                           "mulmodm1_precomp": mp.mulmodm1_stage_kernels(L, depth, w, mp.M1_PRE)},
               "workspace_bytes": {"mul": mp.workspace_bytes(L, L, md, mw), "mulmod": mp.mulmod_workspace_bytes(L, depth, w),
                                   "mulmodm1": mp.mulmodm1_workspace_bytes(L, depth, w, mp.M1_MUL),
                                   "sqrmodm1": mp.mulmodm1_workspace_bytes(L, depth, w, mp.M1_SQR),
                                   "mulmodm1_precomp": mp.mulmodm1_workspace_bytes(L, depth, w, mp.M1_PRE),
                                   "cache": mp.mulmodm1_precomp_bytes(L, depth, w)},
               "ms": {k: stats(v) for k, v in t.items()}}
        med = {k: row["ms"][k]["median"] for k in t}
        row["ratio_mulmodm1_to_mulmod"] = med["mulmodm1"] / med["mulmod"]
        row["ratio_mulmodm1_to_mul"] = med["mulmodm1"] / med["mul"]
        row["ratio_precomp_to_mulmodm1"] = med["mulmodm1_precomp"] / med["mulmodm1"]
        row["ratio_sqrmodm1_to_mulmodm1"] = med["sqrmodm1"] / med["mulmodm1"]
        saved = med["mulmodm1"] - med["mulmodm1_precomp"]
        row["precomp_break_even_products"] = med["precomp"] / saved if saved > 0 else None
        row["stages_ms"] = {k: profiled(mp, entries[k], torch) for k in ("mul", "mulmod", "mulmodm1", "sqrmodm1", "mulmodm1_precomp")}
    print(json.dumps(row), flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else None
    if out:
        with open(out, "w") as f:
            json.dump([row], f, indent=1)
    assert all(same.values()), same

    def bar(x, y):
        m = max(row["ms"][x]["spread"], row["ms"][y]["spread"])
        assert med[x] <= med[y] + m, "%s %.3f ms above %s %.3f ms (margin %.3f)" % (x, med[x], y, med[y], m)
    bar("mulmodm1", "mulmod")
    bar("mulmodm1_precomp", "mulmodm1")
    bar("sqrmodm1", "mulmodm1")


if __name__ == "__main__":
    main()
