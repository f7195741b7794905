#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# round 4, call O: the tight k_pwss (K = 512 in 80 KiB of LDS, two workgroups per CU;
# libmpfft_tight.so, -DPW_TIGHT9=1) -- parity at l = 4096, then C4 A/B against the shipped one
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT
MPFFT_LIB=libmpfft_tight.so timeout -k 10 600 python -u -m pytest -x -v --timeout 300 --timeout-method thread tests/test_gpu_parity.py -m gpu -k "4096 or nested or fill_fold" > $OUT/pytest_tight.log 2>&1 || { tail -40 $OUT/pytest_tight.log; exit 1; }
tail -2 $OUT/pytest_tight.log
for v in main tight main tight; do
  if [ $v = main ]; then unset MPFFT_LIB; else export MPFFT_LIB=libmpfft_tight.so; fi
  timeout -k 10 300 python3 bench.py --full --config C4 --steps 3 --warmup 1 --no-cpu-baseline --no-twin --e2e-reps 0 > $OUT/tight_C4_$v.log 2>&1 || exit 1
  python3 -c "
import json
d=json.loads([x for x in open('$OUT/tight_C4_$v.log') if x.startswith('{')][-1]); print('C4 $v', round(d['ms_per_step'],2), d.get('exact'), 'pointwise', round(d['stages_ms']['pointwise'],2))"
done
