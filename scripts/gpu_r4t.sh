#!/bin/bash
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/out}   # OUT: where this run's logs go
# round 4, call T: rocprofv3 kernel statistics of the driver's bench command itself (N = 1:
# C3 + the C4 twin), to set beside the line's roofline.avg_ms for k_pwss
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/ks_default -o c -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $OUT/ks_default.log 2>&1 || { tail -20 $OUT/ks_default.log; exit 1; }
grep '^{' $OUT/ks_default.log | python3 -c "
import json,sys; d=json.loads(sys.stdin.read().splitlines()[-1]); r=d['roofline']; print('bench', round(d['ms_per_step'],3), r['kernel'], 'avg_ms', round(r['avg_ms'],4), 'frac', round(r['frac'],4))"
python3 scripts/kstats.py $OUT/ks_default 8
