"""Cost of the nav driver and of the prompt fetch.  Prints one JSON line.  Run on the GPU box.

  python tools/rx_nav_time.py step --case parent|nav [--signal FILE.npy]
      The tests/lock_cases.py run (four L1 C/A channels, 8 s at 4.092 Msps in 32 pushes of 0.25 s, the lock monitor on,
      steps of up to 300 periods).  Per push the host wall time, the ring transfer waited for beforehand, of
        parent: gnsscorr_rx_step + gnsscorr_trk_fetch + gnsscorr_trk_fetch_log, the fetches a caller's loop needs;
                touches no nav entry point, so it also runs on the library of the commit before (GNSSCORR_LIB);
        nav:    gnsscorr_rx_nav_step alone (step, log, prompt column, status, feed).
      One process measures one case; run the cases in alternating processes.  --signal: a cache file for the synthetic
      IF (made when missing).

  python tools/rx_nav_time.py prompt
      gnsscorr_trk_fetch_prompt against gnsscorr_trk_fetch (II and QQ, no nsamp) behind one closed-loop run, at 5 and at
      33 taps, for 4 channels x 300 periods and 32 x 400: mean host wall time of PROMPT_REPS = 200 calls each,
      alternating in blocks of 20."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gnsscorr_loader  # noqa: E402

REPS = int(os.environ.get("PROMPT_REPS", "200"))


def lock_signal(gc, lc, path):
    import importlib
    synth = importlib.import_module("erlangnetwork_gnsslib_sdr_amd.synth")
    n = lc.NCHUNK * lc.CHUNK
    if path and os.path.exists(path):
        data = np.load(path)
        if data.shape == (n, 2) and data.dtype == np.int8:
            return data
    data = lc.signal(gc, synth)
    if path:
        tmp = "%s.%d.tmp" % (path, os.getpid())
        with open(tmp, "wb") as f:
            np.save(f, data)
        os.replace(tmp, path)
    return data


def step_times(gc, case, path):
    import lock_cases as lc
    sig = lock_signal(gc, lc, path)
    eng = gc.Engine(0)
    eng.ring_create(1, 2, 2 * lc.CHUNK)
    eng.set_channels(lc.channels(gc))
    eng.loop_set([eng.loop_state(i, 0.0) for i in range(len(lc.PRNS))])
    eng.rx_start(lc.RETRY_MS)
    for i, p in enumerate(lc.PRNS):
        eng.rx_lock_set(lc.prm_of(p), ch0=i, nch=1)
    if case == "nav":
        eng.rx_nav_start(10, 2)
    us, periods = [], 0
    for k in range(lc.NCHUNK):
        eng.ring_push_raw(1, sig[k * lc.CHUNK:(k + 1) * lc.CHUNK], lc.CHUNK)
        eng.ring_read(1, (k + 1) * lc.CHUNK - 16, 16, 2)        # the ring transfer is over
        t0 = time.perf_counter()
        if case == "nav":
            eng.rx_nav_step(lc.MAX_PERIODS)
        else:
            eng.rx_step(lc.MAX_PERIODS)
            eng.trk_fetch()
            eng.trk_fetch_log()
        us.append(1e6 * (time.perf_counter() - t0))
        periods += int(eng.trk_fetch_log()[1].sum())
    out = {"case": case, "steps": len(us), "periods": periods, "total_ms": round(sum(us) / 1e3, 2),
           "us_per_step_median": round(float(np.median(us)), 1), "us_per_step_mean": round(float(np.mean(us)), 1),
           "us_per_period": round(sum(us) / max(periods, 1), 3)}
    if case == "nav":
        st = eng.rx_nav().status(len(lc.PRNS))
        out["nrows"], out["resets"] = [int(v) for v in st["nrows"]], [int(v) for v in st["resets"]]
    eng.close()
    return out


def prompt_times(gc):
    out = {"reps": REPS}
    rng = np.random.default_rng(1)
    for corrn in (2, 16):
        for nch, nper in ((4, 300), (32, 400)):
            n = 4092 * (nper + 8)
            eng = gc.Engine(0)
            eng.ring_create(1, 2, n)
            eng.ring_push_raw(1, rng.integers(-60, 61, size=(n, 2), dtype=np.int8), n)
            chans = [gc.Channel(p, dtype=2, f_sf=4.092e6, f_if=0.0, corrn=corrn, corrd=1, corrp=1) for p in range(1, nch + 1)]
            eng.set_channels(chans)
            eng.trk_set_state([dict(carrfreq=100.0 * i, codefreq=c.crate, remcode=0.0, remcarr=0.0, buffloc=16 + i) for i, c in enumerate(chans)])
            eng.loop_set([eng.loop_state(i, 100.0 * i) for i in range(nch)])
            eng.trk_run_loop(nper)
            II, QQ, _ = eng.trk_fetch()
            II0, QQ0 = eng.trk_fetch_prompt()
            assert II0.tobytes() == np.ascontiguousarray(II[:, :, 0]).tobytes() and QQ0.tobytes() == np.ascontiguousarray(QQ[:, :, 0]).tobytes()
            L, h = gc.lib(), eng.h
            t = {"fetch": 0.0, "prompt": 0.0}
            for _ in range(REPS // 20):
                t0 = time.perf_counter()
                for _ in range(20):
                    L.gnsscorr_trk_fetch(h, II.ctypes.data, QQ.ctypes.data, None)
                t1 = time.perf_counter()
                for _ in range(20):
                    L.gnsscorr_trk_fetch_prompt(h, II0.ctypes.data, QQ0.ctypes.data)
                t2 = time.perf_counter()
                t["fetch"] += t1 - t0
                t["prompt"] += t2 - t1
            calls = 20 * (REPS // 20)
            out["taps%d_nch%d_nper%d" % (2 * corrn + 1, nch, nper)] = {
                "trk_fetch_us": round(1e6 * t["fetch"] / calls, 1), "trk_fetch_prompt_us": round(1e6 * t["prompt"] / calls, 1),
                "doubles_fetch": int(II.size + QQ.size), "doubles_prompt": int(II0.size + QQ0.size)}
            eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "prompt"])
    ap.add_argument("--case", choices=["parent", "nav"], default="nav")
    ap.add_argument("--signal", default=None)
    a = ap.parse_args()
    gc = gnsscorr_loader.load()
    print(json.dumps(step_times(gc, a.case, a.signal) if a.what == "step" else prompt_times(gc)))


if __name__ == "__main__":
    main()
