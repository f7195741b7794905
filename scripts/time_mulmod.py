#!/usr/bin/env python3
"""MI355X timing of the products mod 2^B + 1 next to the only other route to the residue, the
full product: mulmod_device(a, b), sqrmod_device(a) and mul_device(a, b) of the L-limb operands
at choose(L, L)'s pair (before its host fold and its 2 L-limb transfer).  First the mulmod result
is checked for equality with that product folded on the host.  Each entry is warmed up once, then
20 calls on one stream between HIP events, the three alternating for three rounds each; reports
the median and the spread (max - min) of the rounds, the ratios, and one profiled call's per-stage
times (profile_begin / profile_end).
Cases: the full-efficiency shape (14, 8), L = 33 550 336 (l = 2048, 32 768 slots), and a Fermat-type
modulus, L = 2^24 at mulmod_choose's pair (pieces of N/4 bits: no gain in slots expected).
usage: python scripts/time_mulmod.py [out.json]"""
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
    """the 2 L-limb product mod 2^(64 L) + 1 as an integer: low half minus high half"""
    v = int.from_bytes(prod.tobytes(), "little")
    B = 64 * L
    return ((v & ((1 << B) - 1)) - (v >> B)) % ((1 << B) + 1)


def stats(t):
    return {"median": statistics.median(t), "spread": max(t) - min(t), "rounds": t}


def main():
    import torch
    import mpfft_loader
    mp = mpfft_loader.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    rows = []
    cases = [("full", 33550336, (14, 8)), ("fermat", 1 << 24, mp.mulmod_choose(1 << 24))]
    for name, L, (depth, w) in cases:
        md, mw = mp.choose(L, L)
        a, b = mp.fill_random(L + 1, 0x1001), mp.fill_random(L + 1, 0x2002)
        a[L] = b[L] = 0
        da = torch.from_numpy(a.view(np.int64)).to(dev)
        db = torch.from_numpy(b.view(np.int64)).to(dev)
        del a, b
        dm = torch.zeros(2 * L, dtype=torch.int64, device=dev)
        dr = torch.zeros(L + 1, dtype=torch.int64, device=dev)
        ds = torch.zeros(L + 1, dtype=torch.int64, device=dev)
        wsm = mp.alloc_workspace(L, L, md, mw, dev)
        wsr = mp.alloc_workspace_mulmod(L, depth, w, False, dev)
        wss = mp.alloc_workspace_mulmod(L, depth, w, True, dev)
        mul = lambda: mp.mul_device(dm, da, L, db, L, md, mw, wsm, stream=stream)
        mod = lambda: mp.mulmod_device(dr, da, db, L, depth, w, wsr, stream=stream)
        sqr = lambda: mp.sqrmod_device(ds, da, L, depth, w, wss, stream=stream)
        with torch.cuda.stream(stream):
            mul()
            mod()
            sqr()
            torch.cuda.synchronize()
            want = fold(dm.cpu().numpy().view(np.uint64), L)
            same = int.from_bytes(dr.cpu().numpy().tobytes(), "little") == want
            del want
            tm, tr, ts = [], [], []
            for _ in range(ROUNDS):
                tm.append(timed(mul, torch, stream))
                tr.append(timed(mod, torch, stream))
                ts.append(timed(sqr, torch, stream))
            row = {"name": name, "L": L, "mulmod": {"depth": depth, "w": w, **mp.mulmod_plan_info(L, depth, w)},
                   "mul": {"depth": md, "w": mw, **mp.plan_info(L, L, md, mw)}, "same_residue": same,
                   "kernels": {"mulmod": mp.mulmod_stage_kernels(L, depth, w), "mul": mp.stage_kernels(L, L, md, mw)},
                   "workspace_bytes": {"mul": mp.workspace_bytes(L, L, md, mw), "mulmod": mp.mulmod_workspace_bytes(L, depth, w),
                                       "sqrmod": mp.mulmod_workspace_bytes(L, depth, w, True)},
                   "mul_ms": stats(tm), "mulmod_ms": stats(tr), "sqrmod_ms": stats(ts)}
            row["ratio_mulmod_to_mul"] = row["mulmod_ms"]["median"] / row["mul_ms"]["median"]
            row["ratio_sqrmod_to_mulmod"] = row["sqrmod_ms"]["median"] / row["mulmod_ms"]["median"]
            row["stages_ms"] = {"mul": profiled(mp, mul, torch), "mulmod": profiled(mp, mod, torch),
                                "sqrmod": profiled(mp, sqr, torch)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        assert same, "mulmod_device differs from the folded product at %s" % name
        del wsm, wsr, wss, dm, dr, ds, da, db
        torch.cuda.empty_cache()
    out = sys.argv[1] if len(sys.argv) > 1 else None
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
    # acceptance: at the full-efficiency shape the residue costs no more than the whole product
    full = rows[0]
    assert full["ratio_mulmod_to_mul"] <= 1.0, "mulmod slower than the full multiply: ratio %.3f" % full["ratio_mulmod_to_mul"]


if __name__ == "__main__":
    main()
