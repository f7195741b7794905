#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# Per-kernel counters for profiles/pmc_<CFG>.json: FETCH_SIZE, WRITE_SIZE and two SQ limiter sets,
# each in a rocprofv3 --pmc pass of its own over `bench.py --config <CFG> --steps 1 --warmup 0`.
# usage: scripts/gpu_pmc_all.sh C3 [C4 ...]
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT || exit 1
for CFG in "$@"; do
  B="python3 bench.py --full --config $CFG --steps 1 --warmup 0 --no-cpu-baseline --no-check --e2e-reps 0 --no-twin"
  for P in "f:FETCH_SIZE" "w:WRITE_SIZE" \
           "sqa:SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_INSTS_VALU GRBM_GUI_ACTIVE" \
           "sqb:SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VALU_INT64 SQ_INSTS_VALU GRBM_GUI_ACTIVE"; do
    t=${P%%:*}; c=${P#*:}
    timeout -s KILL 240 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc_${CFG}_$t -o c -- $B > $OUT/pmc_${CFG}_$t.log 2>&1 || exit 1
    python3 scripts/pmc_summary.py $OUT/pmc_${CFG}_$t $OUT/pmc_${CFG}_$t.json > /dev/null || exit 1
  done
  python3 scripts/pmc_merge.py $CFG $OUT/pmc_${CFG}_f.json $OUT/pmc_${CFG}_w.json $OUT/pmc_$CFG.json \
      $OUT/pmc_${CFG}_sqa.json $OUT/pmc_${CFG}_sqb.json || exit 1
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/ks_$CFG -o c -- python3 bench.py --full --config $CFG --steps 3 --warmup 1 --no-cpu-baseline --no-check --e2e-reps 0 --no-twin > $OUT/ks_$CFG.log 2>&1 || exit 1
  echo "== $CFG"; python3 scripts/kstats.py $OUT/ks_$CFG 12
done
