#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# GPU suite, then the C3 bench for each k_combine1 block size (MPFFT_CB_V).
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT && \
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 && \
for v in 1 2 4 8; do MPFFT_CB_V=$v timeout -k 10 200 python3 -u bench.py --full --steps 10 --no-cpu-baseline --e2e-reps 0 > $OUT/bench_cbv$v.log 2>&1 || exit 1; done
rc=$?; echo "rc=$rc"; tail -2 $OUT/pytest_gpu.log
for v in 1 2 4 8; do python3 -c "import json,sys; d=json.loads(open('$OUT/bench_cbv$v.log').read().strip().splitlines()[-1]); print($v, round(d['ms_per_step'],3), d['exact'], {k: round(x,3) for k,x in d['stages_ms'].items()})" ; done
exit $rc
