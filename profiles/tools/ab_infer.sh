#!/bin/bash
# same-box A/B of two environments on the sliding-window inference leg (512^3, one member): ab_infer.sh "ENV_A" "ENV_B" [repeats]
A=$1; B=$2; N=${3:-2}
log=$(mktemp); trap 'rm -f "$log"' EXIT
for i in $(seq $N); do
  for E in "$A" "$B"; do
    env $E python bench.py --full --no-fp32 --no-cpu-baseline --steps 1 --warmup 0 --referee-epochs 0 --weights he > "$log" 2>&1
    python - "$E" "$log" <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[2]) if l.startswith("{")][-1])
i = d["inference"]
print(f"[{sys.argv[1] or 'default'}] feature-space {i['seconds']} s ({i['ms_per_window']} ms/window, {i['frac_of_mfma_peak']} of peak); fp32 logits accumulator {i['fp32_logits_accumulator']['seconds']} s", flush=True)
PY
  done
done
