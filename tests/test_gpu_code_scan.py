"""The batch planner's code chain as a scan (gnsscorr_plan.hip: plan4_code_wave, trk_spec_kernel's scan rows;
gnsscorr_nco.h: gc_code_scan_row / gc_code_scan_next) on the GPU.

6 channels -- rising, falling, +9 kHz, -9 kHz, the exact chip rate from remcode 0 (its sums hit their thresholds
exactly: no brackets), and a fresh state with remcode 0.7 (first period on the cs >= 0 side) -- over back-to-back
batches of 1, 63, 64, 65 and 130 periods (blocks of 64: every remainder) and one more batch after trk_set_state.
Sample counts, sums and the final state equal the oracle's sdrtracking() bit for bit; the scan counter
(gnsscorr_debug_plan_scan) says the bracketed channels were served by the scan; and a fresh process with
GNSSCORR_PLAN_VERIFY=1 -- the checked chain for every period, the scan's proposals held against it -- returns the
same arrays with gc_plan_stats[6] == 0."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 63, 64, 65, 130)
AFTER = 70                                      # the batch after trk_set_state
NS = 16368
NSAMP = NS * (sum(BATCHES) + AFTER + 8)
SEED = 6262
PRNS = (2, 7, 13, 21, 26, 30)


def _states(crates, second=False):
    carr = (2345.5, -1777.25, 9000.0, -9000.0, 1000.0, 512.5)
    doff = (1.3, -2.1, 5.9, -5.9, 0.0, 0.4)
    remcode = (0.31, 0.62, 0.05, 0.93, 0.0, 0.7)
    remcarr = (1.0, -40.0, 3.0, -2000.0, 0.0, 0.5)
    return [dict(carrfreq=carr[i] + (7.0 if second else 0.0), codefreq=crates[i] + doff[i], remcode=remcode[i] + (0.01 * i if second else 0.0),
                 remcarr=remcarr[i], buffloc=(900 if second else 40) + 11 * i) for i in range(6)]


SCRIPT = f"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, {ROOT!r})
sys.path.insert(0, {os.path.dirname(os.path.abspath(__file__))!r})
import gnsscorr_loader
from test_gpu_code_scan import _states, BATCHES, AFTER, NSAMP, SEED, PRNS
gc = gnsscorr_loader.load()
data = np.random.default_rng(SEED).integers(-60, 61, size=(NSAMP, 2), dtype=np.int8)
eng = gc.Engine(0)
eng.ring_create(1, 2, NSAMP)
eng.ring_push_raw(1, data, NSAMP)
chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3) for p in PRNS]
eng.set_channels(chans)
crates = [c.crate for c in chans]
stats, scan = np.zeros(8, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
gc.lib().gnsscorr_debug_plan_stats(C.c_void_p(stats.ctypes.data), 1)
gc.lib().gnsscorr_debug_plan_scan(C.c_void_p(scan.ctypes.data), 1)
arr, fins = {{}}, []
for leg, (st, batches) in enumerate(((_states(crates), BATCHES), (_states(crates, True), (AFTER,)))):
    eng.trk_set_state(st)
    for k, nb in enumerate(batches):
        eng.trk_run(nb)
        II, QQ, ns = eng.trk_fetch()
        arr[f"II_{{leg}}_{{k}}"], arr[f"QQ_{{leg}}_{{k}}"], arr[f"ns_{{leg}}_{{k}}"] = II.copy(), QQ.copy(), ns.copy()
    fins.append([[f["remcode"].hex(), f["remcarr"].hex(), int(f["buffloc"])] for f in eng.trk_get_state()])
gc.lib().gnsscorr_debug_plan_stats(C.c_void_p(stats.ctypes.data), 1)
assert gc.lib().gnsscorr_debug_plan_scan(C.c_void_p(scan.ctypes.data), 1) == 0
np.savez(sys.argv[1], **arr)
print(json.dumps(dict(fins=fins, stats=stats.tolist(), scan=scan[:8].tolist())))
"""


@pytest.mark.gpu
def test_code_scan_against_oracle_and_verify_mode(gc, orc, tmp_path):
    script = tmp_path / "run.py"
    script.write_text(SCRIPT)
    runs = {}
    for mode, env_add in (("default", {}), ("verify", {"GNSSCORR_PLAN_VERIFY": "1"})):
        env = {k: v for k, v in os.environ.items() if k not in ("GNSSCORR_PLAN_VERIFY", "GNSSCORR_TRK_NOSPEC")}
        env.update(env_add)
        npz = tmp_path / f"{mode}.npz"
        r = subprocess.run([sys.executable, str(script), str(npz)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (mode, r.returncode, r.stderr[-3000:])
        runs[mode] = (json.loads(r.stdout.strip().splitlines()[-1]), dict(np.load(npz)))
    d, v = runs["default"], runs["verify"]
    print("default", d[0]["stats"], d[0]["scan"], "verify", v[0]["stats"], v[0]["scan"])
    # verify mode: same results, no proposal of the scan (and no bracketed step) differs from the checked chain
    assert v[0]["fins"] == d[0]["fins"]
    assert sorted(v[1]) == sorted(d[1])
    for k in d[1]:
        assert np.array_equal(v[1][k], d[1][k]), k
    assert v[0]["stats"][6] == 0 and d[0]["stats"][6] == 0, (v[0]["stats"], d[0]["stats"])
    # the oracle, literally
    data = np.random.default_rng(SEED).integers(-60, 61, size=(NSAMP, 2), dtype=np.int8)
    ring = orc.make_ring(data, NSAMP, NSAMP)
    chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3) for p in PRNS]
    crates = [c.crate for c in chans]
    for leg, (states, batches) in enumerate(((_states(crates), BATCHES), (_states(crates, True), (AFTER,)))):
        for i, (c, st) in enumerate(zip(chans, states)):
            o = orc.make_chan(c.prn, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3)
            o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
            b = st["buffloc"]
            for k, nb in enumerate(batches):
                II, QQ, ns = d[1][f"II_{leg}_{k}"], d[1][f"QQ_{leg}_{k}"], d[1][f"ns_{leg}_{k}"]
                for e in range(nb):
                    orc.lib().orc_sdrtracking(C.byref(o), C.byref(ring), b)
                    assert ns[i, e] == o.currnsamp, (leg, i, k, e)
                    assert np.array_equal(II[i, e], np.ctypeslib.as_array(o.II)[:5]), (leg, i, k, e)
                    assert np.array_equal(QQ[i, e], np.ctypeslib.as_array(o.QQ)[:5]), (leg, i, k, e)
                    b += o.currnsamp
            fin = d[0]["fins"][leg][i]
            assert fin[0] == o.remcode.hex() and fin[1] == o.remcarr.hex() and fin[2] == b, (leg, i)
    # who served the periods: code and carrier tallies equal (whole batches of 6 channels); the scan served the
    # bracketed channels -- all but a few periods of the four random-rate channels (the CPU chains of
    # tests/test_nco_code_scan.py: at least 90 %; here less one period per batch planned, which may be an unbracketed
    # first period), some of the channel that starts on the cs >= 0 side
    for meta in (d[0], v[0]):
        st, sc = meta["stats"], meta["scan"]
        code, car = st[0] + st[1] + st[2], st[3] + st[4] + st[5]
        assert code == car and code % 6 == 0, st
        P = code // 6
        assert P >= sum(BATCHES) + AFTER
        for ch in (0, 1, 2, 3):
            assert sc[ch] >= 0.9 * P - 2 * (len(BATCHES) + 1), (ch, sc, P)
        assert sc[5] > 0, sc
        assert not any(sc[6:]), sc
