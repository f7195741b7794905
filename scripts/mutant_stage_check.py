"""Run the mutants of scripts/mutant_stage.sh (GPU): for each, the random-operand stage test as it
was before the adversarial stage tests (run_stages with the forward / pointwise / inverse / combine
checks) and then with its two newer boundary checks, and tests/test_gpu_stage_adversarial.py, all
at the mutant's shapes.  Every run is a fresh process (the library is chosen by MPFFT_LIB at
import).  Prints one line per run; wanted: a mutant the old check passes and the new tests kill.

    python scripts/mutant_stage_check.py [out-file]
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = os.path.join(ROOT, "mpir-fft_amd")
# mutant -> rows of stage_model.TABLE
MUTANTS = {"wave_canon": ("wave-l48", "wave-l256"), "wave_top": ("wave-l48", "wave-l256"),
           "rp_carry": ("rpass-l1024-a", "rpass-l2048-b")}

OLD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests"); sys.path.insert(0, {root!r} + "/oracle")
import mpfft_loader, oracle
from gpu_stages import run_stages
mp = mpfft_loader.load()
d, w, n = {d}, {w}, {n}
a = mp.fill_random(n, 1000 + d * 7 + n)
b = mp.fill_random(n, 2000 + w * 3 + n)
f = run_stages(mp, d, w, a, b, check={check!r}, mul=oracle.gmp_mul)
print("\\n".join(x[:200] for x in f[:3]))
sys.exit(1 if f else 0)
"""


def run(cmd, lib):
    env = dict(os.environ, MPFFT_LIB=lib)
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    # a device fault is no failing check: report it as a crash, which ends the whole run
    bad = any(w in r.stdout for w in ("illegal memory access", "HIP error", "hipError", "Aborted", "Segmentation"))
    return (70 if bad and r.returncode in (0, 1) else r.returncode), r.stdout


def main():
    import stage_model as sm
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout

    def say(s):
        print(s, file=out, flush=True)
        if out is not sys.stdout:
            print(s, flush=True)

    for name, rows in MUTANTS.items():
        lib = os.path.join(PKG, f"libmpfft_mut_{name}.so")
        if not os.path.exists(lib):
            say(f"{name}: {lib} not built (scripts/mutant_stage.sh)")
            continue
        for rid in rows:
            row = next(r for r in sm.TABLE if r["id"] == rid)
            d, w, n = row["depth"], row["w"], sm.table_n(row)
            for label, check in (("test_stages_exact, the checks before this change", ("fwd", "pw", "inv", "comb")),
                                 ("test_stages_exact with the fwdc and invr checks", ("fwdc", "fwd", "pw", "invr", "inv", "comb"))):
                rc, txt = run([sys.executable, "-c", OLD.format(root=ROOT, d=d, w=w, n=n, check=check)], lib)
                if rc not in (0, 1):   # not a failing check: a crash ends the whole run
                    say(f"{name} {rid}: {label}: exit {rc}\n{txt[-2000:]}")
                    return 2
                say(f"{name} {rid} ({d}, {w}, {n}): {label}: {'PASSES (mutant survives)' if rc == 0 else 'FAILS (mutant killed)'}")
                for line in txt.strip().splitlines()[:2]:
                    say("      " + line[:200])
            rc, txt = run([sys.executable, "-m", "pytest", "-q", "-x", "--no-header", "-p", "no:cacheprovider",
                           "tests/test_gpu_stage_adversarial.py", "-k", rid], lib)
            if rc not in (0, 1):
                say(f"{name} {rid}: adversarial tests: exit {rc}\n{txt[-2000:]}")
                return 2
            say(f"{name} {rid}: tests/test_gpu_stage_adversarial.py -k {rid}: {'PASSES (mutant survives)' if rc == 0 else 'FAILS (mutant killed)'}")
            for line in [x for x in txt.splitlines() if x.startswith(("FAILED", "E  ")) or " passed" in x or " failed" in x][:4]:
                say("      " + line[:240])
    return 0


if __name__ == "__main__":
    sys.exit(main())
