"""Bit synchronisation by symbol energy: times.  Prints one JSON line.  Run on the GPU box.

  python tools/bsync_time.py kernel
      HIP-event time of rx_bsync (gnsscorr_timing, mean of BSYNC_REPS = 50 launches through gnsscorr_bsync_run) for
      32 channels x 1000 rows at rate 20, the detector testing every 25 symbols and never deciding (the whole walk).

  python tools/bsync_time.py step --case parent|off|on [--signal FILE.npy]
      Host wall time per period of gnsscorr_rx_step by DESIGN 6's recipe (tools/lock_time.py's: BASELINE's 32 channels,
      a 100-period warm-up step that acquires and hands over, then 5 steps of 400 periods).  off: the schedule without
      gnsscorr_rx_bsync_set; on: the detector on for all 32 channels with a gate nothing passes, so that every launch
      walks all its rows; parent: the same calls as off and no bsync entry point touched, so that the script also runs
      in a checkout of the commit before the detector.  One process measures one case; alternate the cases.

  python tools/bsync_time.py coldstart --case off|on [--signal FILE.npy]
      A 32-channel cold start (PRN 1 .. 32, int8 IQ at 4.092 Msps, synth.default_sats: ten satellites present, random
      50 bit/s data) in pushes of 0.25 s with one step each, up to the step in which the last tracking channel is
      synchronised (or 5 s): seconds of signal per second of wall time over those steps, the push and a
      gnsscorr_loop_get per step included.  on: the detector with start_cnt 200, 50 symbols per test, up to 200, gate
      1.5."""
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

REPS = int(os.environ.get("BSYNC_REPS", "50"))
NCH = lock_time.NCH
COLD_F_SF, COLD_NSAMP, COLD_SECONDS = 4.092e6, 4092, 5.0
COLD_PRM = dict(start_cnt=200, nsym=50, nsym_max=200, gate=1.5)


def kernel_times(gc):
    eng = gc.Engine(0)
    nch, nper = 32, 1000
    rng = np.random.default_rng(1)
    I = rng.integers(-2 ** 25, 2 ** 25, size=(nch, nper)) / 32.0
    Q = rng.integers(-2 ** 25, 2 ** 25, size=(nch, nper)) / 32.0
    log = np.zeros((nch, nper), dtype=np.dtype(gc.TrkLog))
    prm = np.zeros(nch, dtype=np.dtype(gc.BsyncPrm))
    prm["start_cnt"], prm["nsym"], prm["nsym_max"], prm["gate"] = 0, 25, 4096, 1e9
    args = (prm, np.full(nch, 20, np.int32), None, I, Q, log, np.full(nch, nper, np.int32), np.full(nch, 5000, np.uint64))
    run = lambda: eng.bsync_run(args[0], args[1], np.zeros(nch, dtype=np.dtype(gc.BsyncState)), *args[3:])
    for _ in range(3):
        run()
    eng.timing(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    for _ in range(REPS):
        st = run()
    wall = (time.perf_counter() - t0) / REPS
    eng.timing(False)
    ms, n = eng.timing_read("rx_bsync")
    eng.close()
    return {"reps": REPS, "nch%d_nper%d" % (nch, nper): {"rx_bsync_us": round(1e3 * ms / max(n, 1), 2), "launches": n,
                                                           "bsync_run_wall_us": round(1e6 * wall, 1), "tests": int(st["tests"].sum())}}


def step_times(gc, case, path):
    WARM, CALL, NCALL, NSAMP = lock_time.WARM, lock_time.CALL, lock_time.NCALL, lock_time.NSAMP
    sig = lock_time.bench_signal(gc, path)
    eng = gc.Engine(0)
    chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3) for p in range(1, NCH + 1)]
    first = (WARM + 12) * NSAMP
    eng.ring_create(1, 2, 2 * CALL * NSAMP)
    eng.set_channels(chans)
    eng.loop_set([eng.loop_state(i, 0.0) for i in range(NCH)])
    eng.rx_start()
    if case == "on":
        eng.rx_bsync_set(dict(start_cnt=0, nsym=25, nsym_max=4096, gate=1e9))
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
    out["tracking"] = sum(s["state"] == gc.CH_TRACK for s in eng.rx_status())
    if case == "on":
        st, applied = eng.rx_bsync_status()
        out["tests"], out["applied"] = int(st["tests"].sum()), int(applied.sum())
    eng.close()
    return out


def cold_signal(gc, path):
    import importlib
    synth = importlib.import_module("erlangnetwork_gnsslib_sdr_amd.synth")
    n = int(COLD_SECONDS * COLD_F_SF)
    if path and os.path.exists(path):
        data = np.load(path)
        if data.shape == (n, 2) and data.dtype == np.int8:
            return data
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in range(1, 33)}
    sats = synth.default_sats(list(range(1, 33)), seed=synth.SEED)
    data = synth.make_if(codes, n, f_sf=COLD_F_SF, f_if=0.0, dtype=2, sats=sats, seed=synth.SEED)
    if path:
        tmp = "%s.%d.tmp" % (path, os.getpid())
        with open(tmp, "wb") as f:
            np.save(f, data)
        os.replace(tmp, path)
    return data


def cold_start(gc, case, path):
    sig = cold_signal(gc, path)
    chunk = int(0.25 * COLD_F_SF)
    eng = gc.Engine(0)
    eng.ring_create(1, 2, 2 * chunk)
    eng.set_channels([gc.Channel(p, dtype=2, f_sf=COLD_F_SF, f_if=0.0, corrn=2, corrd=3, corrp=3) for p in range(1, NCH + 1)])
    eng.loop_set([eng.loop_state(i, 0.0) for i in range(NCH)])
    eng.rx_start()
    if case == "on":
        eng.rx_bsync_set(COLD_PRM)
    out = {"case": case, "step_ms": [], "synced": []}
    for k in range(sig.shape[0] // chunk):
        t0 = time.perf_counter()
        eng.ring_push_raw(1, sig[k * chunk:(k + 1) * chunk], chunk)
        eng.rx_step(300)
        loops = eng.loop_get()
        out["step_ms"].append(round(1e3 * (time.perf_counter() - t0), 2))
        track = [i for i, s in enumerate(eng.rx_status()) if s["state"] == gc.CH_TRACK]
        out["synced"].append(sum(loops[i].flagsync != 0 for i in track))
        if track and out["synced"][-1] == len(track):
            break
    out["tracking"] = len(track)
    out["signal_s"] = 0.25 * len(out["step_ms"])
    out["wall_s"] = round(1e-3 * sum(out["step_ms"]), 4)
    out["signal_s_per_s"] = round(out["signal_s"] / out["wall_s"], 2)
    if case == "on":
        st, applied = eng.rx_bsync_status()
        out["applied"] = int(applied.sum())
        out["done"] = [int(x) for x in st["done"][track]]
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "step", "coldstart"])
    ap.add_argument("--case", choices=["parent", "off", "on"], default="off")
    ap.add_argument("--signal", default=None)
    a = ap.parse_args()
    gc = gnsscorr_loader.load()
    if a.what == "kernel":
        out = kernel_times(gc)
    elif a.what == "step":
        out = step_times(gc, a.case, a.signal)
    else:
        out = cold_start(gc, a.case, a.signal)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
