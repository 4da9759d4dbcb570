#!/bin/bash
# rocprofv3 passes for profiles/: kernel stats, then FETCH_SIZE and WRITE_SIZE in separate PMC passes
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
OUT=${OUT:-prof_out}; export OUT; mkdir -p "$OUT"
R=${1:-r1}
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_${R}_stats" -- python3 bench.py --full --steps 4 --warmup 1 --no-cpu > "$OUT/prof_${R}_bench.json" 2> "$OUT/prof_${R}_bench.err"
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$OUT/prof_${R}_fetch" -- python3 bench.py --full --steps 1 --warmup 1 --acq-steps 2 --no-cpu > /dev/null 2> "$OUT/prof_${R}_fetch.err"
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$OUT/prof_${R}_write" -- python3 bench.py --full --steps 1 --warmup 1 --acq-steps 2 --no-cpu > /dev/null 2> "$OUT/prof_${R}_write.err"
find "$OUT" -name "*.csv" | head -20
