#!/bin/bash
# the round's final gate on a GPU box: every -m gpu test, smoke(), the driver's bench command
set -e
out=${OUT_DIR:-out}; mkdir -p "$out"
python -m pytest tests -m gpu -x -q > "$out/gate_tests.log" 2>&1 || { tail -20 "$out/gate_tests.log"; exit 1; }
tail -2 "$out/gate_tests.log"
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$out/gate_smoke.log" 2>&1 || { tail -20 "$out/gate_smoke.log"; exit 1; }
tail -1 "$out/gate_smoke.log"
python bench.py --gpus 1 --steps 20 --warmup 5 --full > "$out/gate_bench.json" 2> "$out/gate_bench.err"
tail -1 "$out/gate_bench.json" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['ecpe_shaped']['ms_per_step'], d['cpu_baseline']['value'])"
