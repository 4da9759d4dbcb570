#!/bin/bash
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
OUT=${OUT:-prof_out}; export OUT; mkdir -p "$OUT"
timeout -k 10 200 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_LDS_BANK_CONFLICT --kernel-trace --output-format csv -d "$OUT/pmc_acq1" -- python3 bench.py --full --steps 1 --warmup 1 --acq-steps 2 --no-cpu > /dev/null 2> "$OUT/pmc_acq1.err"
timeout -k 10 200 rocprofv3 --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_IDX_ACTIVE SQ_INSTS_VMEM_WR --kernel-trace --output-format csv -d "$OUT/pmc_acq2" -- python3 bench.py --full --steps 1 --warmup 1 --acq-steps 2 --no-cpu > /dev/null 2> "$OUT/pmc_acq2.err"
python3 - <<'PY'
import csv,glob,collections,re,os
for d in (os.environ["OUT"]+"/pmc_acq1",os.environ["OUT"]+"/pmc_acq2"):
    for f in glob.glob(d+"/*/*counter_collection.csv"):
        agg=collections.defaultdict(lambda: collections.defaultdict(list))
        for r in csv.DictReader(open(f)):
            m=re.search(r'(\w+_kernel)',r["Kernel_Name"]); k=m.group(1) if m else r["Kernel_Name"][:20]
            agg[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
        for k in ("acq_corr_kernel",):
            for c,v in agg[k].items(): print(k,c,"%.4g"%(sum(v)/len(v)))
PY
