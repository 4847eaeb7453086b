#!/bin/bash
# round 5: same-box A/B of the default bench step under environment switches.  usage: r06_ab.sh TAG "ENV1" "ENV2" ... (each ENV is a
# string of VAR=value pairs, "" = defaults); every variant runs twice, interleaved
cd "$GRAFT_REPO_ROOT" || exit 1
O=${AB_OUT:-$(mktemp -d)}  # per-variant JSON lines and stderr logs
mkdir -p "$O"
TAG=$1; shift
for rep in 1 2; do
  i=0
  for E in "$@"; do
    i=$((i+1))
    env $E timeout 600 python bench.py --full --no-cpu-baseline --no-decode --no-other-configs ${BENCH_ARGS} > "$O/ab_${TAG}_${i}_${rep}.json" 2> "$O/ab_${TAG}_${i}_${rep}.err"
    python - "$E" "$O/ab_${TAG}_${i}_${rep}.json" <<'PY'
import json, sys
try:
    d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
    r = d.get("roofline") or {}
    print(f"[{sys.argv[1]:40s}] ms_per_step {d['ms_per_step']:.3f}  gemm_ms {r.get('gemm_ms_per_step', float('nan')):.2f}  frac {r.get('frac', float('nan')):.4f}  loss {d['config']['last_loss_per_sentence']:.3f}")
except Exception as e:
    print(f"[{sys.argv[1]}] FAILED {e}")
PY
  done
done
