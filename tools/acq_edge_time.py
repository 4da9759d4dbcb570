"""Acquisition kernel times with bit-edge hypotheses: HIP-event times of acq_fwd, acq_corr and
acq_final (gnsscorr_timing) and the wall time of one search, for the bench's 32-SV cold search (PRN 1..32, int8 IQ at
16.368 Msps, the bench's signal, +-7 kHz at 50 Hz: 281 bins, intg 10, ncoh 10) with estep 0, 1, 2 and 5 (1, 10, 5 and 2
hypotheses per group).  Prints one JSON line.  Run on the GPU box:

  python tools/acq_edge_time.py [--estep 0,1,2,5] [--batches 5] [--reps 10]
  python tools/acq_edge_time.py --ab PARENT_LIB [--rounds 3]

Every figure is given per batch (the mean over `reps` searches), so that the spread from batch to batch is in the
output.  --ab: the estep 0 search with this tree's library and with PARENT_LIB (a build of the parent commit; it needs
gnsscorr_acq_set_coherent only) in fresh processes that alternate in the order new, parent, parent, new, `rounds`
times over; one JSON line with every process's row."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gnsscorr_loader  # noqa: E402
from acq_coh_time import KERNELS, bench_signal  # noqa: E402

F_SF, NSAMP, NCH, INTG, HBAND, NCOH, STEP = 16.368e6, 16368, 32, 10, 7000, 10, 50


def search_times(gc, sig, estep, batches, reps):
    eng = gc.Engine(0)
    kw = {"estep": estep} if estep else {}
    chans = [gc.Channel(p, dtype=2, f_if=0.0, hband=HBAND, step=STEP, intg=INTG, ncoh=NCOH, **kw)
             for p in range(1, NCH + 1)]
    n = sig.shape[0]
    eng.ring_create(1, 2, n)
    eng.ring_push_raw(1, sig, n)
    eng.set_channels(chans)
    wrpos = (INTG + 1) * NSAMP + NSAMP // 3
    for _ in range(2):
        eng.acq_run(wrpos)
    eng.sync()
    hyps = len(range(0, NCOH, estep)) if estep else 1
    row = {"estep": estep, "hyps": hyps, "nfreq": chans[0].nfreq, "wall_ms": []}
    row.update({k + "_ms": [] for k in KERNELS})
    eng.timing(True)
    for _ in range(batches):
        eng.timing_reset()
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.acq_run(wrpos)
        eng.sync()
        row["wall_ms"].append(round(1e3 * (time.perf_counter() - t0) / reps, 4))
        for k in KERNELS:
            ms, cnt = eng.timing_read(k)
            row[k + "_ms"].append(round(ms / max(cnt, 1), 4))
    eng.timing(False)
    res = eng.acq_fetch()
    row["acquired"] = sorted(c.prn for c, r in zip(chans, res) if r["flagacq"])
    if estep:
        row["edge"] = {c.prn: e for c, e in zip(chans, eng.acq_fetch_edge()) if e >= 0}
    eng.close()
    return row


def alternate(parent_lib, rounds, batches, reps):
    """estep 0 in fresh processes, this tree's library and the parent's alternating (no process here opens the GPU)."""
    rows = []
    for _ in range(rounds):
        for lib in ("new", "parent", "parent", "new"):
            env = dict(os.environ)
            if lib == "parent":
                env["GNSSCORR_LIB"] = os.path.abspath(parent_lib)
            else:
                env.pop("GNSSCORR_LIB", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--estep", "0", "--batches", str(batches),
                                  "--reps", str(reps)], env=env, check=True, capture_output=True, text=True,
                                 timeout=300).stdout
            row = json.loads(out.strip().splitlines()[-1])["estep0"]
            row["lib"] = lib
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--estep", default="0,1,2,5")
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ab", default=None, metavar="PARENT_LIB")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.ab:
        print(json.dumps({"ab": alternate(a.ab, a.rounds, a.batches, a.reps)}))
        return
    gc = gnsscorr_loader.load()
    sig, sats = bench_signal(gc)
    out = {"lib": gc.LIB_PATH, "batches": a.batches, "reps": a.reps,
           "present": {s["prn"]: round(s["cn0"], 1) for s in sats}}
    for k in (int(x) for x in a.estep.split(",")):
        out["estep%d" % k] = search_times(gc, sig, k, a.batches, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
