#!/bin/bash
# Every bench config once with --full (GPU box, repo root) into $BENCH_OUT/bench_all/<config>.json
# (default bench_out/); the default C3 line and C5 with their CPU baselines.
set -euo pipefail
OUT=${BENCH_OUT:-bench_out}/bench_all
mkdir -p "$OUT"
timeout -k 10 300 python bench.py --full > "$OUT/botsort.json" 2> "$OUT/botsort.err"
timeout -k 10 300 python bench.py --full --config boosttrack_mot8 > "$OUT/boosttrack_mot8.json" 2> "$OUT/boosttrack_mot8.err"
for c in botsort_crowded bytetrack ocsort boosttrack strongsort strongsort_c4; do
  timeout -k 10 300 python bench.py --full --config $c --no-cpu-baseline > "$OUT/$c.json" 2> "$OUT/$c.err"
done
timeout -k 10 300 python bench.py --full --config strongsort_c4 --start-frame 150 --no-cpu-baseline > "$OUT/strongsort_c4_steady.json" 2> "$OUT/strongsort_c4_steady.err"
# the C3 line with every frame's outputs delivered to pinned host memory (bench.py --with-d2h)
timeout -k 10 300 python bench.py --full --with-d2h --no-cpu-baseline > "$OUT/botsort_with_d2h.json" 2> "$OUT/botsort_with_d2h.err"
# the multi-GPU entry point on the one-GPU box: two ranks over gloo sharing the card (rehearsal)
BX_DIST_BACKEND=gloo timeout -k 10 300 python bench.py --full --gpus 2 --config boosttrack_mot8 --no-cpu-baseline > "$OUT/boosttrack_mot8_gpus2_gloo.json" 2> "$OUT/boosttrack_mot8_gpus2_gloo.err"
