#!/bin/bash
# serial kernel statistics of the ECPE-shaped step (packed batches, ~1.8 k tokens): rocprofv3 --kernel-trace --stats of bench.py --shape B
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
tag=${1:-rXX}; out=${OUT_DIR:-out}; mkdir -p "$out"
rm -rf "$out/prof_ecpe"
rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof_ecpe" -- python3 bench.py --full --shape B --no-overlap --no-ecpe --no-cpu-baseline --steps 30 --warmup 5 > "$out/${tag}_bench_ecpe_serial_profiled.json" 2> "$out/prof_ecpe.err"
cp "$(find "$out/prof_ecpe" -name '*kernel_stats.csv' | head -1)" "$out/${tag}_bench_ecpe_serial_kernel_stats.csv"
rm -rf "$out/prof_ecpe"
