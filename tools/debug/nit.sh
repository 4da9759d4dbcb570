OUT=${OUT:-prof_out}; export OUT; mkdir -p "$OUT"
for a in 1 2; do
  GNSSCORR_TRK_NIT=$a timeout -k 10 120 python bench.py --full --steps 2 --warmup 1 --inner 8 --no-cpu --no-acq --loop-periods 0 2>/dev/null | tail -1 > "$OUT/nit_$a.json"
  python -c "import json; d=json.load(open('$OUT/nit_$a.json')); print('nit', $a, d['kernels_ms_per_launch'])"
done
