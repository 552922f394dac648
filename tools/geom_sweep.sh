#!/bin/bash
# usage: tools/geom_sweep.sh <tag> "<res:guests> ..."  -- one-wave match finder by launch geometry
tag=$1; shift
out=${FLATE_OUT_ROOT:-results}/$tag
mkdir -p "$out"
for rg in $1; do
  r=${rg%%:*}; g=${rg##*:}
  python3 bench.py --full --steps 5 --warmup 2 --no-extra --cpu-sample-streams 1024 --option resident_blocks=$r --option guest_blocks=$g > "$out/b_${r}_${g}.json" 2> "$out/b_${r}_${g}.err" || echo FAIL $rg
  python3 - <<PY
import json
d=json.loads(open("$out/b_${r}_${g}.json").read().strip().splitlines()[-1])
print("$rg", d["value"], d["config"]["stage_ms"])
PY
done
