OUT=${OUT:-prof_out}; export OUT; mkdir -p "$OUT"
for a in 0 1 2 3; do
  GNSSCORR_TRK_ABLATE=$a timeout -k 10 120 python bench.py --full --steps 2 --warmup 1 --inner 8 --no-cpu --no-acq --loop-periods 0 2>/dev/null | tail -1 > "$OUT/abl_$a.json"
  python -c "import json; d=json.load(open('$OUT/abl_$a.json')); print('ablate', $a, d['kernels_ms_per_launch'])"
done
