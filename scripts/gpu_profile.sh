#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# Evidence for profiles/: rocprofv3 kernel stats of the C3 bench, FETCH/WRITE PMC passes
# (separate runs), and the new_mpn_mul6 bench lines (C3 operands, test_mul4's shape).
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT && \
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 && timeout -k 10 200 python3 -u bench.py --full --steps 10 --no-cpu-baseline --e2e-reps 0 > $OUT/bench_default.log 2>&1 && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/p_c3 -o c3 -- python3 bench.py --full --config C3 --steps 3 --warmup 1 --no-cpu-baseline --no-check --e2e-reps 0 > $OUT/p_c3.log 2>&1 && \
timeout -s KILL 180 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_f -o c3 -- python3 bench.py --full --config C3 --steps 1 --warmup 0 --no-cpu-baseline --no-check --e2e-reps 0 > $OUT/pmc_f.log 2>&1 && \
timeout -s KILL 180 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_w -o c3 -- python3 bench.py --full --config C3 --steps 1 --warmup 0 --no-cpu-baseline --no-check --e2e-reps 0 > $OUT/pmc_w.log 2>&1 && \
python3 scripts/pmc_summary.py $OUT/pmc_f $OUT/pmc_f.json > /dev/null && python3 scripts/pmc_summary.py $OUT/pmc_w $OUT/pmc_w.json > /dev/null && \
timeout -k 10 200 python3 -u bench.py --mul6 --steps 5 > $OUT/bench_mul6_c3.log 2>&1 && \
timeout -k 10 200 python3 -u bench.py --mul6 --config M4 --steps 10 > $OUT/bench_mul6_m4.log 2>&1
rc=$?; echo "rc=$rc"; tail -1 $OUT/bench_mul6_c3.log | cut -c1-400; tail -1 $OUT/bench_mul6_m4.log | cut -c1-400; exit $rc
