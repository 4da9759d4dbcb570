#!/bin/bash
# end-of-round record: GPU suite, default bench, rocprofv3 stats + FETCH/WRITE passes (tools/prof.sh), SQ counters of the correlator
cd "$(dirname "$0")/../.."
OUT=${OUT:-prof_out}; export OUT; mkdir -p "$OUT"
timeout -k 10 600 python -m pytest tests -x -q -m gpu > $OUT/q_tests.log 2>&1 || { tail -30 $OUT/q_tests.log; exit 1; }
tail -2 $OUT/q_tests.log
timeout -k 10 400 python bench.py --full > $OUT/q_bench_default.json 2> $OUT/q_bench_default.err || { tail -20 $OUT/q_bench_default.err; exit 1; }
tail -c 600 $OUT/q_bench_default.json; echo
timeout -k 10 500 bash tools/prof.sh q > $OUT/q_prof.log 2>&1 || { tail -20 $OUT/q_prof.log; exit 1; }
timeout -k 10 400 bash tools/pmc_trk.sh > $OUT/q_pmc_sq_trk_corr.txt 2>&1 || { tail -20 $OUT/q_pmc_sq_trk_corr.txt; exit 1; }
tail -20 $OUT/q_pmc_sq_trk_corr.txt
