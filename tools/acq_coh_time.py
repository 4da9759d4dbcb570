"""Acquisition kernel times with coherent integration: HIP-event times of acq_fwd, acq_corr and
acq_final (gnsscorr_timing) and the wall time of one search, for the bench's 32-SV cold search (PRN 1..32, int8 IQ at
16.368 Msps, the bench's signal, +-7 kHz, intg 10) with ncoh 1, 5 and 10 on grids of 200, 100 and 50 Hz (71, 141 and
281 bins: coherent_step()).  Prints one JSON line.  Run on the GPU box:

  python tools/acq_coh_time.py [--ncoh 1,5,10] [--batches 5] [--reps 10]

Every figure is given per batch (the mean over `reps` searches), so that the spread from batch to batch is in the
output.  For an A/B comparison with another build of the library set GNSSCORR_LIB to it and run the two in alternating
processes; a library from before gnsscorr_acq_set_coherent runs ncoh 1 only (--ncoh 1)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnsscorr_loader  # noqa: E402

F_SF, NSAMP, NCH, INTG, HBAND = 16.368e6, 16368, 32, 10, 7000
KERNELS = ("acq_fwd", "acq_corr", "acq_final")


def bench_signal(gc):
    import importlib
    synth = importlib.import_module("erlangnetwork_gnsslib_sdr_amd.synth")
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in range(1, NCH + 1)}
    sats = synth.default_sats(list(range(1, NCH + 1)), seed=synth.SEED)
    n = (INTG + 2) * NSAMP
    return synth.make_if(codes, n, f_sf=F_SF, f_if=0.0, dtype=2, sats=sats, seed=synth.SEED), sats


def search_times(gc, sig, ncoh, batches, reps):
    eng = gc.Engine(0)
    step = gc.coherent_step(ncoh) if hasattr(gc, "coherent_step") else 200
    kw = {"ncoh": ncoh} if ncoh != 1 else {}
    chans = [gc.Channel(p, dtype=2, f_if=0.0, hband=HBAND, step=step, intg=INTG, **kw) for p in range(1, NCH + 1)]
    n = sig.shape[0]
    eng.ring_create(1, 2, n)
    eng.ring_push_raw(1, sig, n)
    eng.set_channels(chans)
    wrpos = (INTG + 1) * NSAMP + NSAMP // 3
    for _ in range(2):
        eng.acq_run(wrpos)
    eng.sync()
    row = {"step_hz": step, "nfreq": chans[0].nfreq, "groups": INTG // ncoh, "wall_ms": []}
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
    row["iters"] = [r["iters"] for r in res]
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncoh", default="1,5,10")
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    gc = gnsscorr_loader.load()
    sig, sats = bench_signal(gc)
    out = {"lib": gc.LIB_PATH, "batches": a.batches, "reps": a.reps,
           "present": {s["prn"]: round(s["cn0"], 1) for s in sats}}
    for k in (int(x) for x in a.ncoh.split(",")):
        out["ncoh%d" % k] = search_times(gc, sig, k, a.batches, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
