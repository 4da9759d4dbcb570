"""Correlation monitor: times.  Prints one JSON line.  Run on the GPU box.

  python tools/cfm_time.py kernel
      HIP-event time of rx_cfm (gnsscorr_timing, mean of CFM_REPS = 50 launches through gnsscorr_cfm_run) for
      32 channels x 400 rows at rate 20 with 5 and with 33 taps, every row synchronised and a window every 10 bits (the
      whole walk), and the same rows with no row synchronised (nothing but the log is read).  bytes: what the kernel has
      to read once, 2 x 8 x taps per channel-period plus the two log words; GB/s: that over the event time.

  python tools/cfm_time.py step --case parent|off|on [--taps 5|33] [--timed] [--signal FILE.npy]
      Host wall time per period of gnsscorr_rx_step by DESIGN 6's recipe (tools/lock_time.py's: BASELINE's 32 channels,
      a 100-period warm-up step that acquires and hands over, then 5 steps of 400 periods).  off: the schedule without
      gnsscorr_rx_cfm_set; on: the monitor on for all 32 channels with windows from the first bit and tolerances
      nothing fails; parent: the same calls as off and no cfm entry point touched, so that the script also runs in a
      checkout of the commit before the monitor.  --taps 33: corrn 16 at a spacing of one sample (the DLL pair stays at
      3 samples).  --timed: per-kernel timing on, and in the output the HIP-event time of rx_cfm in the warm-up step and
      in each timed step, the rows of the last step that were synchronised, and the mean per launch of rx_cfm, rx_lock
      and rx_bsync (the wall times of such a run carry the events' cost).  One process measures one case; alternate them.
      The channels synchronise about 2020 periods behind their hand-over, so in this recipe the monitor reads data rows
      in the last step only: the rows in front of bit synchronisation cost it the log alone."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnsscorr_loader  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lock_time  # noqa: E402

REPS = int(os.environ.get("CFM_REPS", "50"))
NCH = lock_time.NCH
ON_PRM = dict(kbits=10, skip_bits=0, nbad=2, npair=2, dtol=1e9, rtol=1e9)


def kernel_times(gc):
    eng = gc.Engine(0)
    nch, nper = 32, 400
    out = {"reps": REPS}
    rng = np.random.default_rng(1)
    for corrn in (2, 16):
        ntap = 1 + 2 * corrn
        II = rng.integers(-2 ** 25, 2 ** 25, size=(nch, nper, ntap)) / 32.0
        QQ = rng.integers(-2 ** 25, 2 ** 25, size=(nch, nper, ntap)) / 32.0
        prm = np.zeros(nch, dtype=np.dtype(gc.CfmPrm))
        prm["kbits"], prm["nbad"], prm["npair"], prm["dtol"], prm["rtol"] = 10, 2, corrn, 1e9, 1e9
        for synced in (1, 0):
            log = np.zeros((nch, nper), dtype=np.dtype(gc.TrkLog))
            log["flagsync"] = synced
            for i in range(nch):
                log["navbit"][i, (3 * i) % 20::20] = 1
            run = lambda: eng.cfm_run(prm, np.full(nch, 20, np.int32), corrn, np.zeros(nch, dtype=np.dtype(gc.CfmState)), II, QQ, log,
                                      np.full(nch, nper, np.int32), np.full(nch, 5000, np.uint64))
            for _ in range(3):
                run()
            eng.timing(True)
            eng.timing_reset()
            t0 = time.perf_counter()
            for _ in range(REPS):
                st = run()
            wall = (time.perf_counter() - t0) / REPS
            eng.timing(False)
            ms, n = eng.timing_read("rx_cfm")
            us = 1e3 * ms / max(n, 1)
            nbytes = nch * nper * (8 + (2 * 8 * ntap if synced else 0))
            out["taps%d_%s" % (ntap, "synced" if synced else "unsynced")] = {
                "rx_cfm_us": round(us, 2), "launches": n, "cfm_run_wall_us": round(1e6 * wall, 1), "windows": int(st["windows"].sum()),
                "bytes": nbytes, "GB_per_s": round(nbytes / us * 1e-3, 2)}
    eng.close()
    return out


def step_times(gc, case, path, taps, timed):
    WARM, CALL, NCALL, NSAMP = lock_time.WARM, lock_time.CALL, lock_time.NCALL, lock_time.NSAMP
    sig = lock_time.bench_signal(gc, path)
    eng = gc.Engine(0)
    tapset = dict(corrn=2, corrd=3, corrp=3) if taps == 5 else dict(corrn=16, corrd=1, corrp=3)
    chans = [gc.Channel(p, dtype=2, f_if=0.0, **tapset) for p in range(1, NCH + 1)]
    first = (WARM + 12) * NSAMP
    eng.ring_create(1, 2, 2 * CALL * NSAMP)
    eng.set_channels(chans)
    eng.loop_set([eng.loop_state(i, 0.0) for i in range(NCH)])
    eng.rx_start()
    if case == "on":
        eng.rx_cfm_set(ON_PRM)
    if timed:
        eng.timing(True)
    eng.ring_push_raw(1, sig[:first], first)
    eng.rx_step(WARM)
    eng.sync()
    out = {"case": case, "taps": taps, "timed": bool(timed), "us_per_period": []}
    if timed:
        out["rx_cfm_us"] = [round(1e3 * eng.timing_read("rx_cfm")[0], 2)]       # the warm-up step's launch, then each step's
    at = first
    for _ in range(NCALL):
        n = CALL * NSAMP
        eng.ring_push_raw(1, sig[at:at + n], n)
        at += n
        eng.ring_read(1, at - 16, 16, 2)                        # the ring transfer is over
        before = eng.timing_read("rx_cfm")[0] if timed else 0.0
        t0 = time.perf_counter()
        eng.rx_step(CALL)
        eng.sync()
        out["us_per_period"].append(round(1e6 * (time.perf_counter() - t0) / CALL, 2))
        if timed:
            out["rx_cfm_us"].append(round(1e3 * (eng.timing_read("rx_cfm")[0] - before), 2))
    out["tracking"] = sum(s["state"] == gc.CH_TRACK for s in eng.rx_status())
    if timed:
        log, ndone = eng.trk_fetch_log()
        out["synced_rows_last_step"] = int(sum(int(log["flagsync"][i, :ndone[i]].sum()) for i in range(NCH)))
        for name in ("rx_cfm", "rx_lock", "rx_bsync"):
            ms, n = eng.timing_read(name)
            out[name] = {"us_per_launch": round(1e3 * ms / n, 2) if n else None, "launches": n}
    if case == "on":
        st = eng.rx_cfm_status()
        out["bits"], out["windows"] = int(st["bits"].sum()), int(st["windows"].sum())
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "step"])
    ap.add_argument("--case", choices=["parent", "off", "on"], default="off")
    ap.add_argument("--taps", type=int, choices=[5, 33], default=5)
    ap.add_argument("--timed", action="store_true")
    ap.add_argument("--signal", default=None)
    a = ap.parse_args()
    gc = gnsscorr_loader.load()
    print(json.dumps(kernel_times(gc) if a.what == "kernel" else step_times(gc, a.case, a.signal, a.taps, a.timed)))


if __name__ == "__main__":
    main()
