#!/bin/bash
# same-box A/B of one environment switch over whole epochs: ab_env.sh VAR val_a val_b   (prints epochs/s, ms per epoch)
var=$1; a=$2; b=$3
log=$(mktemp); trap 'rm -f "$log"' EXIT
for v in $a $b $a $b; do
  env $var=$v python bench.py --full --no-fp32 --inference-size 0 --no-cpu-baseline --steps ${AB_STEPS:-3} > "$log" 2>&1
  python - "$var" "$v" "$log" <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[3]) if l.startswith("{")][-1])
print(sys.argv[1], sys.argv[2], d["value"], d["ms_per_step"], d["roofline"]["achieved"])
PY
done
