#!/usr/bin/env python3
"""MI355X timing of the products mod 2^B + 1 with the low-word CRT at the Fermat size L = 2^24
(B = 2^30), in one process: mulmodw_device and sqrmodw_device at mulmodw_choose(L), next to the
yardstick, mulmod_device at mulmod_choose(L), and mul_device at choose(L, L).  First the three
residues are checked for equality (mulmodw against mulmod limb by limb, mulmod against the full
product folded on the host).  Each entry is warmed up once, then 20 calls on one stream between HIP
events, the four alternating for three rounds; reports the median and the spread (max - min) of the
rounds, the ratios, one profiled call's per-stage times (the low-word convolution counts with the
combine stage) and k_nlowconv alone (MPFFT_STAGE_LOWCONV: the clearing of d and the launch) at 2n =
16384, 32768 and 65536, from which the chooser's cost per multiply-add is derived: the marginal
cost between the two larger sizes (CHOOSE_LOWCONV_MAC_NS, plan.hpp).
The bar, asserted: mulmodw_device is faster than mulmod_device by more than the larger of the two
spreads.
usage: python scripts/time_mulmodw.py [out.json]   (default profiles/r16/mulmodw_ab.json)"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, ROUNDS = 20, 3
L = 1 << 24


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
    depth, w = mp.mulmodw_choose(L)
    d0, w0 = mp.mulmod_choose(L)
    md, mw = mp.choose(L, L)
    a, b = mp.fill_random(L + 1, 0x1001), mp.fill_random(L + 1, 0x2002)
    a[L] = b[L] = 0
    da = torch.from_numpy(a.view(np.int64)).to(dev)
    db = torch.from_numpy(b.view(np.int64)).to(dev)
    del a, b
    dm = torch.zeros(2 * L, dtype=torch.int64, device=dev)
    dr, dr0, ds = (torch.zeros(L + 1, dtype=torch.int64, device=dev) for _ in range(3))
    wsm = mp.alloc_workspace(L, L, md, mw, dev)
    wsr = mp.alloc_workspace_mulmodw(L, depth, w, False, dev)
    wss = mp.alloc_workspace_mulmodw(L, depth, w, True, dev)
    ws0 = mp.alloc_workspace_mulmod(L, d0, w0, False, dev)
    mul = lambda: mp.mul_device(dm, da, L, db, L, md, mw, wsm, stream=stream)
    modw = lambda: mp.mulmodw_device(dr, da, db, L, depth, w, wsr, stream=stream)
    mod0 = lambda: mp.mulmod_device(dr0, da, db, L, d0, w0, ws0, stream=stream)
    sqrw = lambda: mp.sqrmodw_device(ds, da, L, depth, w, wss, stream=stream)
    with torch.cuda.stream(stream):
        mul()
        modw()
        mod0()
        sqrw()
        torch.cuda.synchronize()
        same = bool(torch.equal(dr, dr0))
        same_full = int.from_bytes(dr0.cpu().numpy().tobytes(), "little") == fold(dm.cpu().numpy().view(np.uint64), L)
        tw, t0, tm, ts = [], [], [], []
        for _ in range(ROUNDS):
            tw.append(timed(modw, torch, stream))
            t0.append(timed(mod0, torch, stream))
            tm.append(timed(mul, torch, stream))
            ts.append(timed(sqrw, torch, stream))
        row = {"L": L, "mulmodw": {"depth": depth, "w": w, **mp.mulmodw_plan_info(L, depth, w)},
               "mulmod": {"depth": d0, "w": w0, **mp.mulmod_plan_info(L, d0, w0)},
               "mul": {"depth": md, "w": mw, **mp.plan_info(L, L, md, mw)},
               "same_as_mulmod": same, "mulmod_same_as_folded_product": same_full,
               "kernels": {"mulmodw": mp.mulmodw_stage_kernels(L, depth, w), "mulmod": mp.mulmod_stage_kernels(L, d0, w0)},
               "workspace_bytes": {"mulmodw": mp.mulmodw_workspace_bytes(L, depth, w), "mulmod": mp.mulmod_workspace_bytes(L, d0, w0),
                                   "mul": mp.workspace_bytes(L, L, md, mw)},
               "mulmodw_ms": stats(tw), "mulmod_ms": stats(t0), "mul_ms": stats(tm), "sqrmodw_ms": stats(ts)}
        row["ratio_mulmodw_to_mulmod"] = row["mulmodw_ms"]["median"] / row["mulmod_ms"]["median"]
        row["ratio_mulmodw_to_mul"] = row["mulmodw_ms"]["median"] / row["mul_ms"]["median"]
        row["ratio_sqrmodw_to_mulmodw"] = row["sqrmodw_ms"]["median"] / row["mulmodw_ms"]["median"]
        row["stages_ms"] = {"mulmodw": profiled(mp, modw, torch), "mulmod": profiled(mp, mod0, torch),
                            "mul": profiled(mp, mul, torch), "sqrmodw": profiled(mp, sqrw, torch)}
        # k_nlowconv alone: the stage entry on the workspace of each shape
        conv = []
        for cd, cw in ((13, 16), (14, 4), (15, 1)):
            ws = mp.alloc_workspace_mulmodw(L, cd, cw, False, dev)
            lc = lambda: mp.mulmodw_stage(mp.STAGE_LOWCONV, da, db, dr0, L, cd, cw, ws, stream=stream)
            lc()
            torch.cuda.synchronize()
            t = [timed(lc, torch, stream) for _ in range(ROUNDS)]
            macs = float(2 << cd) ** 2
            conv.append({"depth": cd, "w": cw, "macs": macs, "ms": stats(t), "ns_per_mac": statistics.median(t) * 1e6 / macs})
            del ws
        row["lowconv"] = conv
        row["lowconv_marginal_ns_per_mac"] = ((conv[2]["ms"]["median"] - conv[1]["ms"]["median"]) * 1e6
                                              / (conv[2]["macs"] - conv[1]["macs"]))
        row["lowconv_share_of_mulmodw"] = next(c["ms"]["median"] for c in conv if c["depth"] == depth) / row["mulmodw_ms"]["median"] \
            if any(c["depth"] == depth for c in conv) else None
    print(json.dumps(row), flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r16", "mulmodw_ab.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(row, f, indent=1)
    assert same, "mulmodw_device differs from mulmod_device"
    assert same_full, "mulmod_device differs from the folded product"
    # the bar: faster than the plain family by more than the larger spread
    gain = row["mulmod_ms"]["median"] - row["mulmodw_ms"]["median"]
    assert gain > max(row["mulmod_ms"]["spread"], row["mulmodw_ms"]["spread"]), \
        "mulmodw %.3f ms against mulmod %.3f ms: no gain beyond the spread" % (row["mulmodw_ms"]["median"], row["mulmod_ms"]["median"])


if __name__ == "__main__":
    main()
