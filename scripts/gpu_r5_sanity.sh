#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# Round-5 start: the GPU suite and the default bench line at HEAD on a fresh box.
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT && T=${1:-r5a} && \
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -q --timeout 600 --timeout-method thread > $OUT/pytest_$T.log 2>&1 && \
tail -2 $OUT/pytest_$T.log && \
timeout -k 10 600 python3 -u bench.py --full --no-cpu-baseline > $OUT/bench_default_$T.log 2>&1
rc=$?; echo "rc=$rc"; tail -3 $OUT/pytest_$T.log; tail -c 1500 $OUT/bench_default_$T.log; exit $rc
