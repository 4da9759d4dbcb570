"""SBAS frame path times: HIP-event time of fec_viterbi27 for 1, 500 and 4300 full windows (1512 symbols ->
750 bits) on 1 and 8 channels, whole and with the forward pass / the chainback alone (gnsscorr_debug_fec_parts), the
wall time of gnsscorr_fec_run around it, the wall time of a whole sbasframe_replay over 8.6 s of log (a stream that
holds a frame, and noise, where every symbol is decoded and searched), and one decode by the plain C restatement
tools/fec_ref.c (gcc -O2, one thread) on this host.  Prints one JSON line.  Run on the GPU box: python tools/fec_time.py"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gnsscorr_loader  # noqa: E402
import fec_restate as fr  # noqa: E402
import sbas_cases as sc  # noqa: E402

REPS = int(os.environ.get("FEC_REPS", "50"))
NSYM = 4300                                        # 8.6 s of a channel's log at 500 symbols per second


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def main():
    gc = gnsscorr_loader.load()
    eng = gc.Engine(0)
    out = {"reps": REPS, "host_cpu": cpu_model()}
    rng = np.random.default_rng(1)
    for nch in (1, 8):
        sym = (1 - 2 * rng.integers(0, 2, size=(nch, fr.WIN + NSYM))).astype(np.int8)
        for npos in (1, 500, NSYM):
            row = {}
            for parts, tag in ((3, "kernel_ms"), (1, "forward_ms"), (2, "chainback_ms")):
                eng.debug_fec_parts(parts)
                for _ in range(3):
                    eng.fec_run(sym, fr.WIN, npos, rowbytes=fr.ROWBYTES)
                eng.timing(True)
                eng.timing_reset()
                t0 = time.perf_counter()
                for _ in range(REPS):
                    eng.fec_run(sym, fr.WIN, npos, rowbytes=fr.ROWBYTES)
                wall = (time.perf_counter() - t0) / REPS
                eng.timing(False)
                ms, n = eng.timing_read("fec_viterbi27")
                row[tag] = round(ms / max(n, 1), 4)
                if parts == 3:
                    row["fec_run_wall_ms"] = round(1e3 * wall, 3)
            eng.debug_fec_parts(3)
            out["nch%d_npos%d" % (nch, npos)] = row
    # a whole replay: 8600 periods of log
    msgs = [fr.sbas_message(i, 12 if i == 0 else 2 + i, rng.integers(0, 2, size=212), tow=sc.TOW if i == 0 else None,
                            week=sc.WEEK) for i in range(9)]
    streams = {"frame": fr.sbas_stream(msgs)[:NSYM], "noise": (1 - 2 * rng.integers(0, 2, size=NSYM)).astype(np.int8)}
    for name, s in streams.items():
        navbit, buffloc, _, _ = fr.log_columns(s, 0, 0)
        log = np.zeros(len(navbit), dtype=np.dtype(gc.TrkLog))
        log["navbit"], log["buffloc"] = navbit, buffloc
        walls = []
        for _ in range(12):
            st = gc.SbasFrameState()
            t0 = time.perf_counter()
            eng.sbasframe_replay(st, log)
            walls.append(time.perf_counter() - t0)
        out["replay_%s_wall_ms" % name] = round(1e3 * float(np.mean(walls[2:])), 3)
        out["replay_%s_found" % name] = int(st.flagdec)
    eng.close()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "fec_ref")
        subprocess.check_call(["gcc", "-O2", "-o", exe, os.path.join(ROOT, "tools", "fec_ref.c")])
        subprocess.check_output([exe, "50"])
        out["host_c_one_decode_us"] = round(float(subprocess.check_output([exe, "400"]).split()[0]) / 1e3, 2)
    out["host_c_4300_decodes_ms"] = round(out["host_c_one_decode_us"] * NSYM / 1e3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
