"""Acquisition kernel times with code-Doppler compensation: HIP-event times of acq_fwd, acq_corr and
acq_final (gnsscorr_timing) and the wall time of one search, for the bench's 32-SV cold search (PRN 1..32, int8 IQ at
16.368 Msps, the bench's signal, +-7 kHz at 200 Hz: 71 bins, intg 10, ncoh 1) without compensation and with the L1
carrier (acq_fwd's compensating instance: the same kernel plus one load per workgroup).  Prints one JSON line.  Run on
the GPU box:

  python tools/acq_slip_time.py [--cdop 0,1] [--batches 5] [--reps 10]
  python tools/acq_slip_time.py --ab PARENT_LIB [--rounds 3]

Every figure is given per batch (the mean over `reps` searches), so that the spread from batch to batch is in the
output.  --ab: the search without compensation with this tree's library and with PARENT_LIB (a build of the parent
commit) in fresh processes that alternate in the order new, parent, parent, new, `rounds` times over, then this tree's
library with compensation on, `rounds` processes; one JSON line with every process's row and, per figure, the spread
(min, median, max over the processes' batch means) of the parent, of the new library off and of the new library on, and
whether the off median lies inside the parent's spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gnsscorr_loader  # noqa: E402
from acq_coh_time import KERNELS, bench_signal  # noqa: E402

F_SF, NSAMP, NCH, INTG, HBAND, STEP, F_CF = 16.368e6, 16368, 32, 10, 7000, 200, 1575.42e6
FIGURES = tuple(k + "_ms" for k in KERNELS) + ("wall_ms",)


def search_times(gc, sig, cdop, batches, reps):
    eng = gc.Engine(0)
    kw = {"cdop": True, "f_cf": F_CF} if cdop else {}
    chans = [gc.Channel(p, dtype=2, f_if=0.0, hband=HBAND, step=STEP, intg=INTG, **kw) for p in range(1, NCH + 1)]
    n = sig.shape[0]
    eng.ring_create(1, 2, n)
    eng.ring_push_raw(1, sig, n)
    eng.set_channels(chans)
    wrpos = (INTG + 1) * NSAMP + NSAMP // 3
    for _ in range(2):
        eng.acq_run(wrpos)
    eng.sync()
    row = {"cdop": int(cdop), "nfreq": chans[0].nfreq, "wall_ms": []}
    if cdop:
        s, back = eng.acq_fetch_shifts(0)
        row.update(back=back, shift_min=int(s.min()), shift_max=int(s.max()))
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
    eng.close()
    return row


def _process(lib, parent_lib, cdop, batches, reps):
    """One search_times in a fresh process (no process here opens the GPU)."""
    env = dict(os.environ)
    if lib == "parent":
        env["GNSSCORR_LIB"] = os.path.abspath(parent_lib)
    else:
        env.pop("GNSSCORR_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cdop", str(cdop), "--batches", str(batches),
                          "--reps", str(reps)], env=env, check=True, capture_output=True, text=True, timeout=300).stdout
    row = json.loads(out.strip().splitlines()[-1])["cdop%d" % cdop]
    row["lib"] = lib
    return row


def _spread(rows, fig):
    means = [statistics.fmean(r[fig]) for r in rows]
    return [round(min(means), 4), round(statistics.median(means), 4), round(max(means), 4)]


def alternate(parent_lib, rounds, batches, reps):
    rows = []
    for _ in range(rounds):
        for lib in ("new", "parent", "parent", "new"):
            rows.append(_process(lib, parent_lib, 0, batches, reps))
    for _ in range(rounds):
        rows.append(_process("new", parent_lib, 1, batches, reps))
    groups = {"parent": [r for r in rows if r["lib"] == "parent"],
              "new_off": [r for r in rows if r["lib"] == "new" and not r["cdop"]],
              "new_on": [r for r in rows if r["lib"] == "new" and r["cdop"]]}
    summary = {}
    for fig in FIGURES:
        s = {k: _spread(v, fig) for k, v in groups.items()}
        s["off_inside_parent_spread"] = s["parent"][0] <= s["new_off"][1] <= s["parent"][2]
        summary[fig] = s
    return {"ab": rows, "summary": summary}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cdop", default="0,1")
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ab", default=None, metavar="PARENT_LIB")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.ab:
        print(json.dumps(alternate(a.ab, a.rounds, a.batches, a.reps)))
        return
    gc = gnsscorr_loader.load()
    sig, sats = bench_signal(gc)
    out = {"lib": gc.LIB_PATH, "batches": a.batches, "reps": a.reps,
           "present": {s["prn"]: round(s["cn0"], 1) for s in sats}}
    for k in (int(x) for x in a.cdop.split(",")):
        out["cdop%d" % k] = search_times(gc, sig, k, a.batches, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
