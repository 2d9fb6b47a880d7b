#!/bin/bash
# Same-box A/B of the in-tree librpt against abl/librpt_base.so (a copy of an earlier build) on
# the bench at FR frames, interleaved: new, base, new, base.  Optional TESTS=... runs first.
# PLAIN=1: the plain bench line (default frames, steps and warm-up, no --full legs; the leg
# switches left on the command act only with --full); also prints steady_state.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
mkdir -p gpurun_out
export HSA_ENABLE_IPC_MODE_LEGACY=0
if [ -n "$TESTS" ]; then
  timeout -k 10 700 python -u -m pytest $TESTS -m gpu -x -q --timeout 300 --timeout-method thread \
    > gpurun_out/gpu_sel.log 2>&1 || { tail -40 gpurun_out/gpu_sel.log; exit 1; }
  tail -2 gpurun_out/gpu_sel.log
fi
FR=${FR:-1000}
BARGS=(--full --total-frames $FR --steps 20 --warmup 3)
[ -n "$PLAIN" ] && BARGS=()
run() {  # tag env...
  local tag=$1; shift
  env "$@" timeout -k 10 240 python bench.py "${BARGS[@]}" \
    --no-cpu-baseline --h2d-steps 0 > gpurun_out/ab_$tag.json 2> gpurun_out/ab_$tag.err || return 1
  python - "$tag" <<'PY'
import json, sys
t = sys.argv[1]
d = json.loads(open(f"gpurun_out/ab_{t}.json").read().strip().splitlines()[-1])
print(t, d["value"], d["ms_per_step"], (d.get("one_stack_in_flight") or {}).get("ms_per_step"),
      d.get("steady_state"), d["stage_ms"])
PY
}
run new1 RPT_AB=new || exit 1
run base1 RPT_LIB=abl/librpt_base.so || exit 1
run new2 RPT_AB=new || exit 1
run base2 RPT_LIB=abl/librpt_base.so || exit 1
if [ -n "$KPROF" ]; then
  bash tools/kprof.sh n$FR --total-frames $FR
  python tools/kstats.py $(find gpurun_out/kprof_n$FR -name "*kernel_stats.csv") 4 > gpurun_out/ks_n.txt
  head -16 gpurun_out/ks_n.txt
fi
