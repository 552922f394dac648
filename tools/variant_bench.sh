#!/bin/bash
# usage: tools/variant_bench.sh <tag> "<opt=val,opt=val> ..."  -- bench lines for sets of engine options
tag=$1; shift
out=${FLATE_OUT_ROOT:-results}/$tag
mkdir -p "$out"
i=0
for set in $1; do
  i=$((i+1))
  opts=""
  for kv in ${set//,/ }; do opts="$opts --option $kv"; done
  python3 bench.py --full --steps 5 --warmup 2 --no-extra --cpu-sample-streams 2048 $opts > "$out/b$i.json" 2> "$out/b$i.err" || echo FAIL $set
  python3 - <<PY
import json
d=json.loads(open("$out/b$i.json").read().strip().splitlines()[-1])
print("$set", d["value"], d["config"]["stage_ms"], d["config"]["parity_checked_streams"])
PY
done
