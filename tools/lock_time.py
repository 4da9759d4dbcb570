"""Lock monitor times.  Prints one JSON line.  Run on the GPU box.

  python tools/lock_time.py kernel
      HIP-event time of rx_lock (gnsscorr_timing, mean of LOCK_REPS = 50 launches through gnsscorr_lock_run) for
      32 channels x 400 periods and 4 x 300: synchronised streams, a nav bit every 20 periods.

  python tools/lock_time.py step --case parent|off|on [--signal FILE.npy]
      Host wall time per period of gnsscorr_rx_step by DESIGN 6's recipe: BASELINE's 32 channels configured (int8 IQ,
      16.368 Msps, the bench's signal), a 100-period warm-up step that acquires and hands over, then 5 steps of 400
      periods, each timed from the call to the end of gnsscorr_sync, the ring transfer waited for beforehand.
      off: the schedule as it is without gnsscorr_rx_lock_set; on: the monitor on for all 32 channels (a threshold no
      tracking channel falls below, so that nothing is sent back to SEARCH); parent: the same calls as off and no
      lock entry point touched, so that the script also runs in a checkout of the commit before the monitor.
      One process measures one case; run each case in two processes, alternating.  --signal: a cache file for the
      synthetic IF (made when missing)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnsscorr_loader  # noqa: E402

REPS = int(os.environ.get("LOCK_REPS", "50"))
F_SF, NSAMP, NCH = 16.368e6, 16368, 32
WARM, CALL, NCALL = 100, 400, 5


def kernel_times(gc):
    eng = gc.Engine(0)
    out = {"reps": REPS}
    rng = np.random.default_rng(1)
    for nch, nper in ((32, 400), (4, 300)):
        I = rng.integers(-2 ** 25, 2 ** 25, size=(nch, nper)) / 32.0
        Q = rng.integers(-2 ** 25, 2 ** 25, size=(nch, nper)) / 32.0
        log = np.zeros((nch, nper), dtype=np.dtype(gc.TrkLog))
        log["flagsync"] = 1
        for i in range(nch):
            log["navbit"][i, (3 * i) % 20::20] = 1
        prm = np.zeros(nch, dtype=np.dtype(gc.LockPrm))
        prm["sync_periods"], prm["kbits"], prm["nbad"], prm["mu_min"] = 2600, 10, 1000000, 5.0
        args = (prm, np.full(nch, 20, np.int32), None, I, Q, log, np.full(nch, nper, np.int32), np.full(nch, 5000, np.uint64))
        run = lambda: eng.lock_run(args[0], args[1], np.zeros(nch, dtype=np.dtype(gc.LockState)), *args[3:])
        for _ in range(3):
            run()
        eng.timing(True)
        eng.timing_reset()
        t0 = time.perf_counter()
        for _ in range(REPS):
            st = run()
        wall = (time.perf_counter() - t0) / REPS
        eng.timing(False)
        ms, n = eng.timing_read("rx_lock")
        out["nch%d_nper%d" % (nch, nper)] = {"rx_lock_us": round(1e3 * ms / max(n, 1), 2), "launches": n,
                                             "lock_run_wall_us": round(1e6 * wall, 1), "windows": int(st["windows"].sum())}
    eng.close()
    return out


def bench_signal(gc, path):
    import importlib
    synth = importlib.import_module("erlangnetwork_gnsslib_sdr_amd.synth")
    n = (WARM + 12 + NCALL * CALL) * NSAMP
    if path and os.path.exists(path):
        data = np.load(path)
        if data.shape == (n, 2) and data.dtype == np.int8:
            return data
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in range(1, 33)}
    sats = synth.default_sats(list(range(1, 33)), seed=synth.SEED)
    data = synth.make_if(codes, n, f_sf=F_SF, f_if=0.0, dtype=2, sats=sats, seed=synth.SEED)
    if path:
        tmp = "%s.%d.tmp" % (path, os.getpid())
        with open(tmp, "wb") as f:
            np.save(f, data)
        os.replace(tmp, path)
    return data


def step_times(gc, case, path):
    sig = bench_signal(gc, path)
    eng = gc.Engine(0)
    chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3) for p in range(1, NCH + 1)]
    first = (WARM + 12) * NSAMP
    eng.ring_create(1, 2, 2 * CALL * NSAMP)
    eng.set_channels(chans)
    eng.loop_set([eng.loop_state(i, 0.0) for i in range(NCH)])
    eng.rx_start()
    if case == "on":
        eng.rx_lock_set(dict(sync_periods=0, kbits=10, nbad=2, mu_min=1e-6))
    eng.ring_push_raw(1, sig[:first], first)
    eng.rx_step(WARM)
    eng.sync()
    out = {"case": case, "us_per_period": []}
    at = first
    for _ in range(NCALL):
        n = CALL * NSAMP
        eng.ring_push_raw(1, sig[at:at + n], n)
        at += n
        eng.ring_read(1, at - 16, 16, 2)                        # the ring transfer is over
        t0 = time.perf_counter()
        eng.rx_step(CALL)
        eng.sync()
        out["us_per_period"].append(round(1e6 * (time.perf_counter() - t0) / CALL, 2))
    st = eng.rx_status()
    _, ndone = eng.trk_fetch_log()
    out["tracking"] = sum(s["state"] == gc.CH_TRACK for s in st)
    out["ndone_last"] = [int(ndone.min()), int(ndone.max())]
    if case == "on":
        lock, losses = eng.rx_lock_status()
        out["losses"] = int(losses.sum())
        out["windows"] = int(lock["windows"].sum())
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "step"])
    ap.add_argument("--case", choices=["parent", "off", "on"], default="off")
    ap.add_argument("--signal", default=None)
    a = ap.parse_args()
    gc = gnsscorr_loader.load()
    print(json.dumps(kernel_times(gc) if a.what == "kernel" else step_times(gc, a.case, a.signal)))


if __name__ == "__main__":
    main()
