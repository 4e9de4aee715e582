#!/bin/bash
# One call: the full bench line (with cpu_baseline, li_ba, ...) + rocprofv3 kernel trace + HBM counter passes of the bench command.
# The bench line goes to $OUT/bench_full.json: pass it to scripts/collect_profile.py as its second argument.
cd "$GRAFT_REPO_ROOT" || exit 1
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout 600 python bench.py --full 2> $OUT/bench_full.err | grep "^{" > $OUT/bench_full.json; echo "bench rc=$? $(wc -c < $OUT/bench_full.json) bytes"; tail -3 $OUT/bench_full.err
STEPS=${STEPS:-90} bash scripts/gpu_profile.sh 2>&1 | tail -8
