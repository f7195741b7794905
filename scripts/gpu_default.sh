#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# The driver's round-end sequence on one GPU: smoke(), then the default bench line (C3, CPU
# baseline, e2e), then its rocprofv3 kernel statistics.
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT && T=${1:-x} && \
timeout -k 10 300 python3 -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke_$T.log 2>&1 && \
timeout -k 10 600 python3 -u bench.py --full > $OUT/bench_default_$T.log 2>&1 && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/ks_$T -o c3 -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-check --e2e-reps 0 > $OUT/ks_$T.log 2>&1
rc=$?; echo "rc=$rc"; tail -2 $OUT/smoke_$T.log; tail -c 3000 $OUT/bench_default_$T.log
python3 scripts/kstats.py $OUT/ks_$T 2>/dev/null | head -12
exit $rc
