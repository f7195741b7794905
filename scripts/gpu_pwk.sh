#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# C4 pointwise with K = 1024 pieces (M = 16, 1024 threads) vs K = 512 (M = 20): pointwise tests
# at l = 4096 and the C4 bench (digest-checked) under MPFFT_PW_LK4096=10 (diagnostic build).
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT && T=${1:-x} && \
MPFFT_LIB=diag MPFFT_PW_LK4096=10 timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -k "pointwise_direct or nested_pointwise or stages_exact" > $OUT/pytest_$T.log 2>&1 && \
MPFFT_LIB=diag MPFFT_PW_LK4096=10 timeout -k 10 300 python3 -u bench.py --full --config C4 --steps 3 --warmup 1 --no-cpu-baseline --e2e-reps 0 > $OUT/bench_c4b_$T.log 2>&1 && \
timeout -k 10 300 python3 -u bench.py --full --config C4 --steps 3 --warmup 1 --no-cpu-baseline --e2e-reps 0 > $OUT/bench_c4_$T.log 2>&1
rc=$?; echo "rc=$rc"; tail -2 $OUT/pytest_$T.log
for c in c4 c4b; do python3 -c "import json; d=json.loads(open('$OUT/bench_${c}_$T.log').read().strip().splitlines()[-1]); print('$c', round(d['ms_per_step'],3), d['exact'], {k: round(x,3) for k,x in d['stages_ms'].items()})" 2>/dev/null; done
exit $rc
