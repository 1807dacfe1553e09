#!/bin/bash
# Round profile set (run on the GPU box): serial kernel stats that the roofline leg must agree with, the overlapped
# default run, and the --full bench line with the CPU baseline.  Outputs land in $OUT_DIR (default out/; copy into profiles/).
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
tag=${1:-rXX}; out=${OUT_DIR:-out}; mkdir -p "$out"
rm -rf "$out/prof_serial" "$out/prof_default"
rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof_serial" -- python3 bench.py --full --no-overlap --no-ecpe --no-cpu-baseline > "$out/${tag}_bench_serial_profiled.json" 2> "$out/prof_serial.err"
cp "$(find "$out/prof_serial" -name '*kernel_stats.csv' | head -1)" "$out/${tag}_bench_serial_kernel_stats.csv"
rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof_default" -- python3 bench.py --full --no-cpu-baseline > "$out/${tag}_bench_default_profiled.json" 2> "$out/prof_default.err"
cp "$(find "$out/prof_default" -name '*kernel_stats.csv' | head -1)" "$out/${tag}_bench_default_kernel_stats.csv"
rm -rf "$out/prof_serial" "$out/prof_default"
python bench.py --full > "$out/${tag}_bench_with_cpu_baseline.json" 2> "$out/bench_default.err"
tail -1 "$out/${tag}_bench_with_cpu_baseline.json" | cut -c1-300
