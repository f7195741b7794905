#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# Round 6: k_pwss's un-weighting folded into the inverse transform's last level (PW_UNW_FUSE=1, libmpfft.so)
# against the separate publish + rotated read (libmpfft_unw0.so): pointwise / product parity through the
# shipped library (and the pw_norm spill-branch build), then C3 x2 / C4 / C2 alternating, rocprof at C3.
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT && L=$ROOT/mpir-fft_amd
rc=0
timeout -k 10 600 python3 -u -m pytest tests/test_gpu_parity.py tests/test_gpu_fold.py tests/test_c_abi.py tests/test_gpu_mul6.py -x -q \
  --timeout 300 --timeout-method thread -m gpu > $OUT/unw_pytest.log 2>&1 || rc=$?
run() {   # tag lib cfg steps
  MPFFT_LIB=$2 timeout -k 10 300 python3 -u bench.py --full --config $3 --steps $4 --warmup 1 \
    --no-cpu-baseline --e2e-reps 0 --no-twin > $OUT/unw_$1.log 2>&1
}
if [ $rc = 0 ]; then
  for rep in 1 2; do
    run c3_old_$rep $L/libmpfft_unw0.so C3 10 || { rc=$?; break; }
    run c3_new_$rep $L/libmpfft.so C3 10 || { rc=$?; break; }
  done
fi
[ $rc = 0 ] && { run c4_old $L/libmpfft_unw0.so C4 3 && run c4_new $L/libmpfft.so C4 3 && run c2_old $L/libmpfft_unw0.so C2 10 && run c2_new $L/libmpfft.so C2 10 || rc=$?; }
[ $rc = 0 ] && { timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/unw_prof -o c -- \
    python3 bench.py --full --config C3 --steps 5 --warmup 1 --no-cpu-baseline --e2e-reps 0 --no-twin > $OUT/unw_prof.log 2>&1 || rc=$?; }
echo "rc=$rc"
tail -n 2 $OUT/unw_pytest.log
for f in $OUT/unw_c*.log; do python3 -c "
import json
d=json.loads([l for l in open('$f') if l.startswith('{')][-1])
print('$f', round(d['ms_per_step'],3), d['exact'], 'pointwise', round(d['stages_ms']['pointwise'],3))" 2>/dev/null || tail -n 3 $f; done
[ $rc = 0 ] && python3 - <<'PY'
import csv
for r in csv.DictReader(open(__import__("os").environ["OUT"] + "/unw_prof/c_kernel_stats.csv")):
    if "k_pwss" in r["Name"]:
        print(r["Name"][:30], r["Calls"], round(float(r["AverageNs"])/1e3,1))
PY
exit $rc
