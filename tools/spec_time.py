"""IF monitor times: HIP-event time of spec_psd / spec_sum / spec_hist for one reference-sized snapshot
(16.368 Msps IQ, SPEC_LEN = 7 ms, nfft 16384, 100 segments) and for 8 in one call, the wall time of a run + fetch
and of the spectrumanalyzer() drop-in, beside the host time of the numpy restatement (one core: numpy's FFT is
single-threaded).  Prints one JSON line.  Run on the GPU box: python tools/spec_time.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gnsscorr_loader  # noqa: E402
import spec_restate as sr  # noqa: E402

F_SF, NFFT, NLOOP = 16.368e6, 16384, 100
N = 7 * 16368
REPS = int(os.environ.get("SPEC_REPS", "50"))


def main():
    gc = gnsscorr_loader.load()
    eng = gc.Engine(0)
    ringlen = 16 * N
    eng.ring_create(2, 2, ringlen)
    data = np.random.default_rng(1).integers(-7, 8, size=(ringlen, 2), dtype=np.int8)
    eng.ring_push(2, data)
    wr = eng.ring_wrpos(2)
    out = {}
    for nsnap in (1, 8):
        locs = [wr - N - 10000 * k for k in range(nsnap)]
        for _ in range(3):
            eng.spectrum(2, locs, N, F_SF, seed=0)
        eng.timing(True)
        eng.timing_reset()
        t0 = time.perf_counter()
        for r in range(REPS):
            eng.spectrum(2, locs, N, F_SF, seed=r)
        wall = (time.perf_counter() - t0) / REPS
        eng.timing(False)
        row = {}
        for k in ("spec_psd", "spec_sum", "spec_hist"):
            ms, n = eng.timing_read(k)
            row[k + "_ms"] = round(ms / max(n, 1), 4)
        row["kernels_ms"] = round(sum(row.values()), 4)
        row["run_fetch_wall_ms"] = round(1e3 * wall, 3)
        out[f"nsnap{nsnap}"] = row
    eng.close()
    snap = data[-N:]
    gc.spectrumanalyzer(snap, 2, F_SF, NFFT)
    t0 = time.perf_counter()
    for _ in range(10):
        gc.spectrumanalyzer(snap, 2, F_SF, NFFT)
    out["dropin_wall_ms"] = round(1e2 * (time.perf_counter() - t0), 3)
    offs = list(np.random.default_rng(0).integers(0, N - NFFT // 2 + 1, size=NLOOP))
    t0 = time.perf_counter()
    sr.spectrumanalyzer(snap, 2, F_SF, NFFT, offs)
    sr.calchistgram(snap, 2, N)
    out["host_numpy_one_snapshot_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
