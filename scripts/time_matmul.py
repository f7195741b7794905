#!/usr/bin/env python3
"""MI355X timing of the small matrix products next to m p sums of products: matmul_device on seeded
operands against m p calls of dot_device(K = k) on the same operands (the dot's code is the parent's:
this feature adds entries and a kernel beside it), at C3 and C2 for 2x2 by 2x2 and 2x2 by 2x1, at the
dot's size for both routes.  Each route is warmed up once, then 20 calls on one stream between HIP
events, the two alternating for three rounds each; reports the median and the spread (max - min) of the
rounds.  First every result entry is checked for equality with its dot_device sum.
The parent's stages, from five profiled calls each (profile_begin / profile_end): F1 = the forward
columns + rows of one operand and X = the k_pwsx stage (precomp_device), S = the k_pwsp stage
(mul_precomp_device), I = inverse rows + columns + scale + combine (mul_device).
k_pwmm alone is timed through matmul_stage on the caches a product left in the workspace, 20 calls
between events, three rounds: one launch for kk = 2 terms (the shipped form) and term by term (kk = 1,
then kk = 1 accumulating: the launches of the fallback form).  The same A/B of the two forms at one shape
of each other inner ring size (M = 20: depth 12, w 64; M = 10: depth 12, w 16 under MPFFT_POINTWISE=pwss),
where nothing else is timed.
Asserted:
1. matmul / (m p dots) <= [(m k + k p) (F1 + X) + m p k S + m p I] / (m p dots) + 0.03: the same product
   term by term against caches, so the inner-domain sum must at least pay for itself;
2. the k_pwmm stage per result entry at kk = 2 is < 2 S.
usage: python scripts/time_matmul.py [out.json]"""
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


def main():
    import torch
    import mpfft_loader
    mp = mpfft_loader.load()
    import mpir_fft_amd.matmul as mmod
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    rows = []
    for name, depth, w, n0 in (("C3", 15, 4, 20312500), ("C2", 15, 4, 15625000)):
        k = 2
        n = min(n0, mp.dot_max_limbs(k, depth, w))
        xs = [torch.from_numpy(mp.fill_random(n, 0x1001 + i).view(np.int64)).to(dev) for i in range(4)]
        ys = [torch.from_numpy(mp.fill_random(n, 0x2002 + i).view(np.int64)).to(dev) for i in range(4)]
        # the parent's stages at this size
        wsm = mp.alloc_workspace(n, n, depth, w, dev)
        wsp = mp.alloc_workspace_mul_precomp(n, n, depth, w, dev)
        pre = mp.alloc_precomp(n, n, depth, w, dev)
        dm = torch.zeros(2 * n, dtype=torch.int64, device=dev)
        with torch.cuda.stream(stream):
            make = lambda: mp.precomp_device(pre, ys[0], n, n, depth, w, wsm, stream=stream)
            mulp = lambda: mp.mul_precomp_device(dm, xs[0], n, pre, n, depth, w, wsp, stream=stream)
            mul = lambda: mp.mul_device(dm, xs[0], n, ys[0], n, depth, w, wsm, stream=stream)
            make(); mulp(); mul()
            torch.cuda.synchronize()
            s_make, s_mulp, s_mul = profiled(mp, make, 1, torch), profiled(mp, mulp, 1, torch), profiled(mp, mul, 1, torch)
        F1, X, S = sum(s_make[f] for f in FWD), s_make["pointwise"], s_mulp["pointwise"]
        I = sum(s_mul[f] for f in INV)
        del wsm, wsp, pre, dm
        torch.cuda.empty_cache()
        for m, p in ((2, 2), (2, 1)):
            X_, Y_ = xs[:m * k], ys[:k * p]
            rs = [torch.zeros(2 * n + 1, dtype=torch.int64, device=dev) for _ in range(m * p)]
            ds = [torch.zeros(2 * n + 1, dtype=torch.int64, device=dev) for _ in range(m * p)]
            wmm = mmod.alloc_workspace_matmul(m, k, p, n, n, depth, w, dev)
            wsd = mp.alloc_workspace_dot(k, n, n, depth, w, dev)

            def dots():
                for i in range(m):
                    for j in range(p):
                        mp.dot_device(ds[i * p + j], [X_[i * k + t] for t in range(k)], [Y_[t * p + j] for t in range(k)],
                                      n, n, depth, w, wsd, stream=stream)
            mm = lambda: mmod.matmul_device(rs, m, k, p, X_, Y_, n, n, depth, w, wmm, stream=stream)
            ea, eb = [0, 1], [m * k, m * k + p]   # result entry (0, 0)
            one = lambda: mmod.matmul_stage(mmod.STAGE_MM_POINTWISE, m, k, p, None, None, None, n, n, depth, w, wmm, ea, eb, stream=stream)

            def termwise():
                mmod.matmul_stage(mmod.STAGE_MM_POINTWISE, m, k, p, None, None, None, n, n, depth, w, wmm, ea[:1], eb[:1], stream=stream)
                mmod.matmul_stage(mmod.STAGE_MM_POINTWISE | mp.STAGE_ACC, m, k, p, None, None, None, n, n, depth, w, wmm, ea[1:], eb[1:],
                                stream=stream)
            with torch.cuda.stream(stream):
                dots()
                mm()
                torch.cuda.synchronize()
                same = all(torch.equal(r, d) for r, d in zip(rs, ds))
                td, tm = [], []
                for _ in range(ROUNDS):
                    td.append(timed(dots, torch, stream))
                    tm.append(timed(mm, torch, stream))
                smm = profiled(mp, mm, m * k + k * p + m * p, torch)
                sdot = profiled(mp, dots, m * p * k, torch)
                # k_pwmm alone on the caches the product left behind
                one(); termwise()
                t1, tt = [], []
                for _ in range(ROUNDS):
                    t1.append(timed(one, torch, stream))
                    tt.append(timed(termwise, torch, stream))
            row = {"name": name, "depth": depth, "w": w, "n": n, "m": m, "k": k, "p": p, "same_as_dots": same,
                   "kernels": mmod.matmul_stage_kernels(m, k, p, n, n, depth, w),
                   "workspace_bytes": {"dot": mp.dot_workspace_bytes(k, n, n, depth, w),
                                       "matmul": mmod.matmul_workspace_bytes(m, k, p, n, n, depth, w)},
                   "dots_ms": stats(td), "matmul_ms": stats(tm),
                   "stages_ms": {"matmul": smm, "dots": sdot, "precomp": s_make, "mul_precomp": s_mulp, "mul": s_mul},
                   "F1": F1, "X": X, "S": S, "I": I,
                   "pwmm_single_ms": stats(t1), "pwmm_termwise_ms": stats(tt)}
            dots_ms = row["dots_ms"]["median"]
            row["ratio"] = row["matmul_ms"]["median"] / dots_ms
            row["predicted"] = ((m * k + k * p) * (F1 + X) + m * p * k * S + m * p * I) / dots_ms
            row["bar"] = row["predicted"] + 0.03
            row["pwmm_over_S"] = row["pwmm_single_ms"]["median"] / S
            row["single_over_termwise"] = row["pwmm_single_ms"]["median"] / row["pwmm_termwise_ms"]["median"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            assert same, "matmul_device differs from dot_device at %s %dx%dx%d" % (name, m, k, p)
            del rs, ds, wmm, wsd
            torch.cuda.empty_cache()
        del xs, ys
        torch.cuda.empty_cache()
    # the two forms of k_pwmm at the other inner ring sizes
    for name, depth, w, kind in (("M20", 12, 64, None), ("M10", 12, 16, "pwss")):
        if kind:
            os.environ["MPFFT_POINTWISE"] = kind
        m = k = p = 2
        n = mp.dot_max_limbs(k, depth, w)
        xs = [torch.from_numpy(mp.fill_random(n, 0x3003 + i).view(np.int64)).to(dev) for i in range(4)]
        ys = [torch.from_numpy(mp.fill_random(n, 0x4004 + i).view(np.int64)).to(dev) for i in range(4)]
        rs = [torch.zeros(2 * n + 1, dtype=torch.int64, device=dev) for _ in range(4)]
        ds = [torch.zeros(2 * n + 1, dtype=torch.int64, device=dev) for _ in range(4)]
        wmm = mmod.alloc_workspace_matmul(m, k, p, n, n, depth, w, dev)
        wsd = mp.alloc_workspace_dot(k, n, n, depth, w, dev)
        ea, eb = [0, 1], [m * k, m * k + p]
        st = lambda which, a, b: mmod.matmul_stage(which, m, k, p, None, None, None, n, n, depth, w, wmm, a, b, stream=stream)
        one = lambda: st(mmod.STAGE_MM_POINTWISE, ea, eb)

        def termwise():
            st(mmod.STAGE_MM_POINTWISE, ea[:1], eb[:1])
            st(mmod.STAGE_MM_POINTWISE | mp.STAGE_ACC, ea[1:], eb[1:])
        with torch.cuda.stream(stream):
            mmod.matmul_device(rs, m, k, p, xs, ys, n, n, depth, w, wmm, stream=stream)
            for i in range(m):
                for j in range(p):
                    mp.dot_device(ds[i * p + j], [xs[i * k + t] for t in range(k)], [ys[t * p + j] for t in range(k)], n, n, depth, w,
                                  wsd, stream=stream)
            torch.cuda.synchronize()
            same = all(torch.equal(r, d) for r, d in zip(rs, ds))
            one(); termwise()
            t1, tt = [], []
            for _ in range(ROUNDS):
                t1.append(timed(one, torch, stream))
                tt.append(timed(termwise, torch, stream))
        row = {"name": name, "depth": depth, "w": w, "n": n, "m": m, "k": k, "p": p, "forms_only": True, "same_as_dots": same,
               "kernels": mmod.matmul_stage_kernels(m, k, p, n, n, depth, w), "live_slots": mp.dot_plan_info(k, n, n, depth, w)["trunc"],
               "pwmm_single_ms": stats(t1), "pwmm_termwise_ms": stats(tt)}
        row["single_over_termwise"] = row["pwmm_single_ms"]["median"] / row["pwmm_termwise_ms"]["median"]
        if kind:
            del os.environ["MPFFT_POINTWISE"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        assert same, "matmul_device differs from dot_device at %s" % name
        del xs, ys, rs, ds, wmm, wsd
        torch.cuda.empty_cache()
    out = sys.argv[1] if len(sys.argv) > 1 else None
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
    late = ["%s %dx%dx%d: %.3f > %.3f" % (r["name"], r["m"], r["k"], r["p"], r["ratio"], r["bar"]) for r in rows if "ratio" in r and r["ratio"] > r["bar"]]
    assert not late, "the matrix product is slower than its bar against m p dots: " + "; ".join(late)
    slow = ["%s %dx%dx%d: %.3f" % (r["name"], r["m"], r["k"], r["p"], r["pwmm_over_S"]) for r in rows if "pwmm_over_S" in r and not r["pwmm_over_S"] < 2.0]
    assert not slow, "k_pwmm's stage per result entry at kk = 2 is not below 2 x k_pwsp's: " + "; ".join(slow)


if __name__ == "__main__":
    main()
