"""The planner chains' value-only steps on the GPU (gnsscorr_plan.hip: gc_carrier_value_step / gc_code_value_step on
the bracketed path, gc_carrier_value_step_one on one-binade periods): 32 channels at Dopplers from -10 to +10 kHz --
grid frequencies, starts within 1e-6 of zero -- over two batches of 1000 periods, run three ways in fresh processes
(default; GNSSCORR_PLAN_VERIFY=1: every step with its checks; GNSSCORR_TRK_NOSPEC=1: the chain that certifies every
step itself).  Everything the batches return must be identical, no bracketed start may fail a check, and a few
channels must equal the oracle's sdrtracking() bit for bit over all periods."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCH, NEPOCH, NBATCH = 32, 1000, 2
NSAMP = 16368 * (NEPOCH * NBATCH + 40)
SEED = 9031


def _states(rng, crates):
    st = []
    for i, crate in enumerate(crates):
        f = -10000.0 + 20000.0 * i / (NCH - 1)
        kind = i % 4
        if kind == 1:
            f = 200.0 * round(f / 200.0)                 # acquisition grid
        remcarr = float(rng.uniform(0.0, 6.2))
        remcode = float(rng.uniform(0.01, 0.99))
        if kind == 2:                                    # starts next to zero
            remcarr = float(rng.uniform(0.0, 1e-6))
            remcode = float(rng.uniform(0.0, 1e-6))
        if kind == 3 and i % 8 == 3:
            remcarr, remcode = 0.0, 0.0
        st.append(dict(carrfreq=f + (float(rng.uniform(-50.0, 50.0)) if kind == 0 else 0.0),
                       codefreq=crate + float(rng.uniform(-4.0, 4.0)), remcode=remcode, remcarr=remcarr,
                       buffloc=int(rng.integers(0, 16368))))
    return st


SCRIPT = f"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, {ROOT!r})
sys.path.insert(0, {os.path.dirname(os.path.abspath(__file__))!r})
import gnsscorr_loader
from test_gpu_value_step import _states, NCH, NEPOCH, NBATCH, NSAMP, SEED
gc = gnsscorr_loader.load()
rng = np.random.default_rng(SEED)
data = rng.integers(-60, 61, size=(NSAMP, 2), dtype=np.int8)
eng = gc.Engine(0)
eng.ring_create(1, 2, NSAMP)
eng.ring_push_raw(1, data, NSAMP)
chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3) for p in range(1, NCH + 1)]
eng.set_channels(chans)
eng.trk_set_state(_states(np.random.default_rng(SEED + 1), [c.crate for c in chans]))
stats = np.zeros(8, dtype=np.uint64)
gc.lib().gnsscorr_debug_plan_stats(C.c_void_p(stats.ctypes.data), 1)
out = []
for b in range(NBATCH):
    eng.trk_run(NEPOCH)
    II, QQ, ns = eng.trk_fetch()
    out.append((II.copy(), QQ.copy(), ns.copy()))
fin = eng.trk_get_state()
gc.lib().gnsscorr_debug_plan_stats(C.c_void_p(stats.ctypes.data), 1)
np.savez(sys.argv[1], II=np.stack([o[0] for o in out]), QQ=np.stack([o[1] for o in out]), ns=np.stack([o[2] for o in out]))
print(json.dumps(dict(fin=[[f["remcode"].hex(), f["remcarr"].hex(), int(f["buffloc"])] for f in fin], stats=stats.tolist())))
"""


@pytest.mark.gpu
def test_value_steps_agree_with_checks_certified_chain_and_oracle(gc, orc, tmp_path):
    script = tmp_path / "run.py"
    script.write_text(SCRIPT)
    runs = {}
    for mode, env_add in (("default", {}), ("verify", {"GNSSCORR_PLAN_VERIFY": "1"}), ("nospec", {"GNSSCORR_TRK_NOSPEC": "1"})):
        env = {k: v for k, v in os.environ.items() if k not in ("GNSSCORR_PLAN_VERIFY", "GNSSCORR_TRK_NOSPEC")}
        env.update(env_add)
        npz = tmp_path / f"{mode}.npz"
        r = subprocess.run([sys.executable, str(script), str(npz)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (mode, r.returncode, r.stderr[-3000:])
        meta = json.loads(r.stdout.strip().splitlines()[-1])
        arr = np.load(npz)
        runs[mode] = (meta, arr["II"], arr["QQ"], arr["ns"])
    d = runs["default"]
    for mode in ("verify", "nospec"):
        m = runs[mode]
        assert m[0]["fin"] == d[0]["fin"], mode
        for k in (1, 2, 3):
            assert np.array_equal(m[k], d[k]), mode
    for mode in ("default", "verify"):
        st = runs[mode][0]["stats"]
        assert st[6] == 0, (mode, st)                   # no bracketed start failed its checks
        assert st[3] >= 0.9 * NCH * NEPOCH * NBATCH, (mode, st)     # the carrier chain evaluated from claims
    # the oracle, literally, for a rising, a falling and a next-to-zero channel over both batches
    rng = np.random.default_rng(SEED)
    data = rng.integers(-60, 61, size=(NSAMP, 2), dtype=np.int8)
    ring = orc.make_ring(data, NSAMP, NSAMP)
    chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3) for p in range(1, NCH + 1)]
    states = _states(np.random.default_rng(SEED + 1), [c.crate for c in chans])
    II, QQ, ns = d[1], d[2], d[3]
    for i in (2, 24, 29):
        st = states[i]
        o = orc.make_chan(chans[i].prn, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3)
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
        b = st["buffloc"]
        for e in range(NEPOCH * NBATCH):
            orc.lib().orc_sdrtracking(C.byref(o), C.byref(ring), b)
            bt, et = divmod(e, NEPOCH)
            assert ns[bt, i, et] == o.currnsamp, (i, e)
            assert np.array_equal(II[bt, i, et], np.ctypeslib.as_array(o.II)[:5]), (i, e)
            assert np.array_equal(QQ[bt, i, et], np.ctypeslib.as_array(o.QQ)[:5]), (i, e)
            b += o.currnsamp
        fin = d[0]["fin"][i]
        assert fin[0] == o.remcode.hex() and fin[1] == o.remcarr.hex() and fin[2] == b, i
