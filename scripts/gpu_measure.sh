#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# Measurements beside the headline: mul6 vs new_mpn_mul timings, single-GPU C4, and the
# k_pwss phase stamps at C3 (diagnostic build path, MPFFT_PW_STAMPS).
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT && \
timeout -k 10 300 python3 -u scripts/time_mul6.py $OUT/mul6_timing.json > $OUT/mul6_timing.log 2>&1 && \
timeout -k 10 300 python3 -u bench.py --full --config C4 --steps 3 --warmup 1 --no-cpu-baseline --e2e-reps 0 > $OUT/bench_c4_single.log 2>&1 && \
MPFFT_PW_STAMPS=1 timeout -k 10 200 python3 -u bench.py --full --config C3 --steps 1 --warmup 0 --no-cpu-baseline --no-check --e2e-reps 0 > $OUT/pw_stamps.log 2>&1
rc=$?; echo "rc=$rc"; cat $OUT/mul6_timing.log | tail -5; tail -1 $OUT/bench_c4_single.log | cut -c1-600; grep pw_stamps $OUT/pw_stamps.log | head -3; exit $rc
