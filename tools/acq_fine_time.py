"""Acquisition times with carrier refinement: HIP-event times of acq_fwd, acq_corr, acq_final and of
the refinement's kernels acq_fine_nco, acq_prompt and acq_fine (gnsscorr_timing), and the wall time of one search, for
the bench's 32-SV cold search (PRN 1..32, int8 IQ at 16.368 Msps, the bench's signal, +-7 kHz on 200 Hz, intg 10) with
nref 0 (off) and 10 on every channel.  With refinement on it also tables, per satellite present, the error of the bin
centre and of the refined frequency against the satellite's carrier, and acq_prompt's read rate (the acquired channels'
nref*nsamp IQ samples over its time).  Prints one JSON line.  Run on the GPU box:

  python tools/acq_fine_time.py [--nref 0,10] [--batches 5] [--reps 10] [--restate]

Every time is given per batch (the mean over `reps` searches), so that the spread from batch to batch is in the
output.  --restate adds the errors of the host restatement (tests/acq_fine_cases.py; needs the oracle built) on the
results the device fetched, and says whether the device's q equal it.  For an A/B comparison with another build of the
library set GNSSCORR_LIB to it and run the two in alternating processes; a library from before gnsscorr_acq_set_refine
runs nref 0 only (--nref 0)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnsscorr_loader  # noqa: E402

F_SF, NSAMP, NCH, INTG, HBAND, STEP = 16.368e6, 16368, 32, 10, 7000, 200
KERNELS = ("acq_fwd", "acq_corr", "acq_final", "acq_fine_nco", "acq_prompt", "acq_fine")


def bench_signal(gc):
    import importlib
    synth = importlib.import_module("erlangnetwork_gnsslib_sdr_amd.synth")
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in range(1, NCH + 1)}
    sats = synth.default_sats(list(range(1, NCH + 1)), seed=synth.SEED)
    n = (INTG + 2) * NSAMP
    return synth.make_if(codes, n, f_sf=F_SF, f_if=0.0, dtype=2, sats=sats, seed=synth.SEED), sats


def restated(gc, sig, chans, res, nref):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as orc
    import acq_cases as ac
    import acq_fine_cases as fc
    out = []
    for c, r in zip(chans, res):
        o = ac.grid(orc.make_chan(c.prn, dtype=2, f_sf=F_SF, f_if=0.0), HBAND, STEP, INTG)
        out.append(fc.fine_freq(orc, o, sig, sig.shape[0], r, nref))
    return out


def search_times(gc, sig, sats, nref, batches, reps, restate):
    eng = gc.Engine(0)
    chans = [gc.Channel(p, dtype=2, f_if=0.0, hband=HBAND, step=STEP, intg=INTG) for p in range(1, NCH + 1)]
    n = sig.shape[0]
    eng.ring_create(1, 2, n)
    eng.ring_push_raw(1, sig, n)
    eng.set_channels(chans)
    if nref:
        eng.acq_set_refine([nref] * NCH)
    wrpos = (INTG + 1) * NSAMP + NSAMP // 3
    for _ in range(2):
        eng.acq_run(wrpos)
    eng.sync()
    row = {"nfreq": chans[0].nfreq, "wall_ms": []}
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
    if nref:
        fine = eng.acq_fetch_fine()
        want = restated(gc, sig, chans, res, nref) if restate else None
        dop = {s["prn"]: s["doppler"] for s in sats}
        row["errors_hz"] = {}
        for i, (c, r, f) in enumerate(zip(chans, res, fine)):
            if r["flagacq"] and c.prn in dop:
                e = {"cn0": round(next(s["cn0"] for s in sats if s["prn"] == c.prn), 1),
                     "coarse": round(r["acqfreq"] - dop[c.prn], 2), "fine": round(f["finefreq"] - dop[c.prn], 2),
                     "quality": round(f["quality"], 3)}
                if want:
                    e["restated"] = round(want[i]["finefreq"] - dop[c.prn], 2)
                    e["q_equal"] = want[i]["q"] == f["q"]
                row["errors_hz"][c.prn] = e
        nbytes = 2.0 * nref * NSAMP * len(row["acquired"])
        ms = sorted(row["acq_prompt_ms"])[len(row["acq_prompt_ms"]) // 2]
        row["acq_prompt_read_gbs"] = round(nbytes / (ms * 1e-3) / 1e9, 2) if ms > 0 else None
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nref", default="0,10")
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--restate", action="store_true")
    a = ap.parse_args()
    gc = gnsscorr_loader.load()
    sig, sats = bench_signal(gc)
    out = {"lib": gc.LIB_PATH, "batches": a.batches, "reps": a.reps,
           "present": {s["prn"]: round(s["cn0"], 1) for s in sats}}
    for k in (int(x) for x in a.nref.split(",")):
        out["nref%d" % k] = search_times(gc, sig, sats, k, a.batches, a.reps, a.restate)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
