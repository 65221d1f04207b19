#!/bin/bash
# launch-overhead measurement (tools/launch_overhead.py), then the 20- and 200-pass bench lines twice each
# (output under $KB_OUT_DIR/lo, default bench_out/lo)
cd "$(dirname "$0")/.."; export TMPDIR=/tmp; O=${KB_OUT_DIR:-bench_out}/lo; mkdir -p $O
KB_LAUNCH_DIAG=1 timeout -k 10 200 python3 tools/launch_overhead.py 3 > $O/auto.json 2> $O/auto.err || { tail $O/auto.err; exit 1; }
cat $O/auto.json
for i in 1 2; do
  for S in 20 200; do
    timeout -k 10 200 python3 bench.py --full --no-cpu-baseline --steps $S --warmup 5 > $O/b${S}_$i.json 2> $O/b${S}_$i.err || { tail $O/b${S}_$i.err; exit 1; }
    python3 -c "import json; d=json.load(open('$O/b${S}_$i.json')); print('bench$S', round(d['value'],1), d['ms_per_step'], d['per_pass_median_ms'], d['python_wall_seconds'], d['device_warmup'])"
  done
done
