#!/usr/bin/env python3
"""MI355X timing of the signed sums of products: sdot_device next to dot_device on the same operands
(the unsigned sum: what the signs cost), next to K calls of mul_device (the route a caller has
without the entry, which would still need a subtraction) and next to a device-to-device
hipMemcpyAsync that moves as many bytes as the pre-pass and the correction move by DESIGN.md 16's
formulas.  dot_device and mul_device are untouched by the feature.  At C3 and C2, K = 2 with one
negative term and K = 4 with two.  First the signed sum is checked against the K products of
mul_device subtracted on the host.  Each route is warmed up once, then 20 calls on one stream
between HIP events, the routes alternating for three rounds each; median and spread (max - min).
Asserted: (a) sdot_device takes less time than the K multiplies; (b) its extra over dot_device is at
most 1.5 x the copy's time -- the gap this project has measured between a latency-bound chained
stream and the pass ceiling (k_combine_red at 3.35 TB/s against about 5 TB/s).
usage: python scripts/time_sdot.py [out.json]"""
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, ROUNDS, PROF_CALLS = 20, 3, 5
MARGIN = 1.5


def model_bytes(n1, n2, negs):
    """bytes read + written by the two added steps: k_sdneg per negative term -- a, b in,
    the scratch, D's limbs and overflow bytes out; from the second one on D in as well -- and k_sdfix
    once: d_r in and out, D's limbs and bytes read twice"""
    first = 16 * n1 + 17 * n2
    later = 16 * n1 + 26 * n2
    fix = 16 * (n1 + n2 + 1) + 18 * n2
    return {"first_negative_term": first, "later_negative_term": later, "correction": fix,
            "total": (first + (negs - 1) * later if negs else 0) + (fix if negs else 0)}


def timed(fn, torch, stream, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def profiled(mp, fn, slots, torch):
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
    hip_copy = mp.lib().hipMemcpyAsync   # the HIP runtime the library is linked with
    hip_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip_copy.restype = ctypes.c_int
    D2D = 3   # hipMemcpyDeviceToDevice
    rows = []
    for name, depth, w, n0 in (("C3", 15, 4, 20312500), ("C2", 15, 4, 15625000)):
        for K, neg in ((2, 0b10), (4, 0b1010)):
            n = min(n0, mp.dot_max_limbs(K, depth, w))
            negs = bin(neg).count("1")
            das = [torch.from_numpy(mp.fill_random(n, 0x1001 + i).view(np.int64)).to(dev) for i in range(K)]
            dbs = [torch.from_numpy(mp.fill_random(n, 0x2002 + i).view(np.int64)).to(dev) for i in range(K)]
            dms = [torch.zeros(2 * n, dtype=torch.int64, device=dev) for _ in range(K)]
            dd = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev)
            ds = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev)
            wsm = mp.alloc_workspace(n, n, depth, w, dev)
            wsd = mp.alloc_workspace_dot(K, n, n, depth, w, dev)
            wss = mp.alloc_workspace_sdot(K, n, n, depth, w, dev)
            mb = model_bytes(n, n, negs)
            half = mb["total"] // 2   # a copy of `half` bytes reads and writes the model's total
            src = torch.empty(half, dtype=torch.uint8, device=dev)
            dst = torch.empty(half, dtype=torch.uint8, device=dev)
            src.fill_(0x5A)

            def muls():
                for i in range(K):
                    mp.mul_device(dms[i], das[i], n, dbs[i], n, depth, w, wsm, stream=stream)
            dot = lambda: mp.dot_device(dd, das, dbs, n, n, depth, w, wsd, stream=stream)
            sdot = lambda: mp.sdot_device(ds, das, dbs, neg, n, n, depth, w, wss, stream=stream)

            def copy():
                rc = hip_copy(dst.data_ptr(), src.data_ptr(), half, D2D, ctypes.c_void_p(stream.cuda_stream))
                assert rc == 0, rc
            with torch.cuda.stream(stream):
                muls()
                dot()
                sdot()
                copy()
                torch.cuda.synchronize()
                prods = [to_int(m) for m in dms]
                same = mp.sdot_to_int(ds.cpu().numpy().view(np.uint64)) == sum(-p if (neg >> i) & 1 else p for i, p in enumerate(prods))
                same_dot = to_int(dd) == sum(prods)
                tm, td, ts, tc = [], [], [], []
                for _ in range(ROUNDS):
                    tm.append(timed(muls, torch, stream))
                    td.append(timed(dot, torch, stream))
                    ts.append(timed(sdot, torch, stream))
                    tc.append(timed(copy, torch, stream))
                pd = profiled(mp, dot, K, torch)
                ps = profiled(mp, sdot, K, torch)
            row = {"name": name, "depth": depth, "w": w, "n": n, "K": K, "neg": neg, "same_signed_sum": same, "same_sum": same_dot,
                   "kernels": mp.sdot_stage_kernels(K, neg, n, n, depth, w),
                   "workspace_bytes": {"dot": mp.dot_workspace_bytes(K, n, n, depth, w), "sdot": mp.sdot_workspace_bytes(K, n, n, depth, w)},
                   "model_bytes": mb, "copy_bytes": half,
                   "muls_ms": stats(tm), "dot_ms": stats(td), "sdot_ms": stats(ts), "copy_ms": stats(tc),
                   "stages_ms": {"dot": pd, "sdot": ps}}
            row["copy_TBps"] = mb["total"] / row["copy_ms"]["median"] / 1e9
            row["sdot_over_dot"] = row["sdot_ms"]["median"] / row["dot_ms"]["median"]
            row["sdot_over_muls"] = row["sdot_ms"]["median"] / row["muls_ms"]["median"]
            row["extra_ms"] = row["sdot_ms"]["median"] - row["dot_ms"]["median"]
            row["extra_budget_ms"] = MARGIN * row["copy_ms"]["median"]
            # the two added phases by the stage events: the pre-passes count with the forward columns, the correction with the combine
            row["prepass_ms"] = ps["fwd_columns"] - pd["fwd_columns"]
            row["correction_ms"] = ps["combine"] - pd["combine"]
            row["a_holds"] = row["sdot_ms"]["median"] < row["muls_ms"]["median"]
            row["b_holds"] = row["extra_ms"] <= row["extra_budget_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            assert same and same_dot, "sdot_device differs from the K products subtracted on the host at %s K = %d" % (name, K)
            del das, dbs, dms, dd, ds, wsm, wsd, wss, src, dst
            torch.cuda.empty_cache()
    out = sys.argv[1] if len(sys.argv) > 1 else None
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
    late = ["%s K=%d: %.3f ms >= %.3f ms" % (r["name"], r["K"], r["sdot_ms"]["median"], r["muls_ms"]["median"]) for r in rows if not r["a_holds"]]
    assert not late, "(a) the signed sum is not faster than K multiplies: " + "; ".join(late)
    over = ["%s K=%d: extra %.3f ms > %.3f ms (pre-pass %.3f, correction %.3f)" % (r["name"], r["K"], r["extra_ms"], r["extra_budget_ms"],
                                                                                 r["prepass_ms"], r["correction_ms"]) for r in rows if not r["b_holds"]]
    assert not over, "(b) the extra over dot_device is above 1.5 x the copy of the model's bytes: " + "; ".join(over)


if __name__ == "__main__":
    main()
