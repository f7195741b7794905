#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# C4 (one GPU): kernel stats and FETCH/WRITE PMC passes (separate runs) -> profiles/pmc_C4.json
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT && \
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/p_c4 -o c4 -- python3 bench.py --full --config C4 --steps 1 --warmup 1 --no-cpu-baseline --no-check --e2e-reps 0 > $OUT/p_c4.log 2>&1 && \
timeout -s KILL 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc4_f -o c4 -- python3 bench.py --full --config C4 --steps 1 --warmup 0 --no-cpu-baseline --no-check --e2e-reps 0 > $OUT/pmc4_f.log 2>&1 && \
timeout -s KILL 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc4_w -o c4 -- python3 bench.py --full --config C4 --steps 1 --warmup 0 --no-cpu-baseline --no-check --e2e-reps 0 > $OUT/pmc4_w.log 2>&1 && \
python3 scripts/pmc_summary.py $OUT/pmc4_f $OUT/pmc4_f.json > /dev/null && python3 scripts/pmc_summary.py $OUT/pmc4_w $OUT/pmc4_w.json > /dev/null
rc=$?; echo "rc=$rc"; exit $rc
