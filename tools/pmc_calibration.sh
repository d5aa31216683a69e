OUT=${BENCH_OUT:-bench_out}/g4
mkdir -p "$OUT" && export TMPDIR=/tmp && \
timeout -k 10 120 ./tools/probes/fetch_calib > "$OUT/calib_plain.txt" 2>&1 && \
timeout -s KILL 90 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/calf" -o run -- ./tools/probes/fetch_calib > "$OUT/calf.log" 2>&1 && \
timeout -s KILL 90 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/calw" -o run -- ./tools/probes/fetch_calib > "$OUT/calw.log" 2>&1 && \
timeout -k 10 400 python -u bench.py --full > "$OUT/bench_botsort.log" 2>&1 && \
timeout -k 10 300 python -u bench.py --full --config botsort_crowded > "$OUT/bench_crowded.log" 2>&1 && \
timeout -k 10 400 python -u bench.py --full --config strongsort_c4 --steps 20 --warmup 5 > "$OUT/bench_c4.log" 2>&1 && \
(timeout -k 10 60 rocprofv3 -L > "$OUT/counters.txt" 2>&1 || true) && \
timeout -s KILL 120 rocprofv3 --pmc SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVES --output-format csv -d "$OUT/mfma_ss" -o run -- python3 bench.py --full --config strongsort --steps 10 --warmup 2 --no-cpu-baseline > "$OUT/mfma_ss.log" 2>&1 && \
timeout -s KILL 120 rocprofv3 --pmc GRBM_GUI_ACTIVE GRBM_COUNT --output-format csv -d "$OUT/grbm_ss" -o run -- python3 bench.py --full --config strongsort --steps 10 --warmup 2 --no-cpu-baseline > "$OUT/grbm_ss.log" 2>&1
echo "rc=$?"
