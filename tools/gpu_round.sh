#!/bin/bash
# One GPU session: diagnostics, GPU tests, bench, rocprof.  Everything lands in $OUT (default: out/).
set -u
cd "$(dirname "$0")/.."
OUT=${OUT:-out}
mkdir -p "$OUT"
export TMPDIR=/tmp
echo "== diag"; timeout 600 python tools/gpu_diag.py > $OUT/diag.log 2>&1; tail -8 $OUT/diag.log
echo "== pytest"; timeout 900 python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu.log 2>&1; tail -15 $OUT/pytest_gpu.log
echo "== bench"; timeout 600 python bench.py --full --steps 100 --warmup 10 --breakdown > $OUT/bench.log 2> $OUT/bench.err; cat $OUT/bench.log; tail -5 $OUT/bench.err
echo "== bench eager"; timeout 600 python bench.py --full --steps 100 --warmup 10 --no-graph --no-cpu-baseline > $OUT/bench_eager.log 2> $OUT/bench_eager.err; cat $OUT/bench_eager.log; tail -3 $OUT/bench_eager.err
echo "== rocprof"; (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats -d "$OLDPWD/$OUT/prof" -o r1 -- python "$OLDPWD/bench.py" --full --steps 50 --warmup 5 --no-graph --no-cpu-baseline > "$OLDPWD/$OUT/rocprof.log" 2>&1); tail -3 $OUT/rocprof.log
find $OUT/prof -name "*stats*" | head; 
f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -30 "$f"
