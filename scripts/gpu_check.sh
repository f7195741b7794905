#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# Round-3 loop: C3 bench (exact vs the GMP digest), C3 kernel stats, then the GPU suite.
# usage: scripts/gpu_check.sh <tag> [pytest -k expression]
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT && T=${1:-x} && \
timeout -k 10 300 python3 -u bench.py --full --steps 10 --cpu-reps 1 --cpu-warmup 0 --e2e-reps 1 > $OUT/bench_$T.log 2>&1 && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/ks_$T -o c3 -- python3 bench.py --full --config C3 --steps 3 --warmup 1 --no-cpu-baseline --no-check --e2e-reps 0 > $OUT/ks_$T.log 2>&1 && \
timeout -k 10 1500 python3 -u -m pytest tests -m gpu -x -v --timeout 600 --timeout-method thread ${2:+-k "$2"} > $OUT/pytest_$T.log 2>&1
rc=$?; echo "rc=$rc"; tail -c 1500 $OUT/bench_$T.log; echo; tail -4 $OUT/pytest_$T.log
python3 scripts/kstats.py $OUT/ks_$T 2>/dev/null
exit $rc
