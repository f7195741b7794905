#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# round 4, call U: the row DIF's last two levels fused into k_pwss (slot quads) at l = 4096 --
# whole GPU suite, then C4 A/B against the pair-less plan (MPFFT_NO_FUSE2, diag library)
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -v --timeout 600 --timeout-method thread > $OUT/pytest_quad.log 2>&1 || { tail -40 $OUT/pytest_quad.log; exit 1; }
tail -2 $OUT/pytest_quad.log
for v in quad none quad none; do
  if [ $v = none ]; then export MPFFT_NO_FUSE2=1; else unset MPFFT_NO_FUSE2; fi
  MPFFT_LIB=diag timeout -k 10 300 python3 bench.py --full --config C4 --steps 3 --warmup 1 --no-cpu-baseline --no-twin --e2e-reps 0 > $OUT/quad_C4_$v.log 2>&1 || exit 1
  python3 -c "
import json
d=json.loads([x for x in open('$OUT/quad_C4_$v.log') if x.startswith('{')][-1]); print('C4 $v', round(d['ms_per_step'],2), d.get('exact'), {k: round(x,2) for k,x in d['stages_ms'].items()})"
done
