#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# Round validation on one MI355X: GPU parity suite, the driver's default bench line,
# and a rocprofv3 kernel-stats pass of the same C3 bench (stops at the first failure).
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT && \
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 && \
timeout -k 10 300 python3 -u bench.py --full > $OUT/bench_default.log 2>&1 && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/p_c3 -o c3 -- python3 bench.py --full --config C3 --steps 3 --warmup 1 --no-cpu-baseline --no-check --e2e-reps 0 > $OUT/p_c3.log 2>&1
rc=$?; echo "rc=$rc"; tail -3 $OUT/pytest_gpu.log; tail -2 $OUT/bench_default.log; exit $rc
