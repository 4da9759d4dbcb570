"""debug: per-channel clocks per period of both planner chains (code, carrier: loop, slow path, waiting for n, in
front of the step, the step) from a library built with -DGC_PLAN_PROF (GNSSCORR_LIB=... for an A/B build); the
planner runs in front of the correlator, alone, 4 x 1000 periods of 32 channels at Dopplers within +-5 kHz.
profiles/r4/*_plan_clocks.txt and profiles/r7/*_plan_clocks.txt are its output.  Since the carrier chain runs on staged
records (profiles/r7): "top" is, per block, the rows, the wait for the code chain's block ("waiting-for-n") and the
staging, divided by the block's periods; "step" the sequential loop; "slow" the clocks in its out-of-line paths."""
import ctypes, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import gnsscorr_loader
gc = gnsscorr_loader.load()
NS, E, NCH, REP = 16368, 1000, 32, 4
rng = np.random.default_rng(20240601)
data = np.random.default_rng(3).integers(-60, 61, size=((E + 4) * NS, 2), dtype=np.int8)
eng = gc.Engine(0)
eng.ring_create(1, 2, data.shape[0]); eng.ring_push_raw(1, data, data.shape[0])
chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3) for p in range(1, NCH + 1)]
eng.set_channels(chans)
st0 = [dict(carrfreq=float(rng.uniform(-5000, 5000)), codefreq=c.crate + float(rng.uniform(-2, 2)), remcode=float(rng.uniform(0.01, 0.99)),
            remcarr=float(rng.uniform(0, 6.2)), buffloc=int(rng.integers(0, NS))) for c in chans]
eng.timing(1)
for rep in range(REP):
    eng.trk_set_state(st0)
    eng.timing_reset()
    eng.trk_run(E)
    eng.sync()
    print("rep", rep, {k: round(eng.timing_read(k)[0] / max(eng.timing_read(k)[1], 1), 4) for k in ("trk_spec", "trk_plan")})
pp = np.zeros(64 * 16, dtype=np.uint64)
gc.lib().gnsscorr_debug_plan_prof(ctypes.c_void_p(pp.ctypes.data))
pp = pp.reshape(64, 2, 8)[:NCH].astype(np.float64) / (REP * E)
print("per period (clocks): ch carrfreq | code loop slow | carrier loop slow waiting-for-n top step | slow periods per launch")
for ch in np.argsort([s["carrfreq"] for s in st0]):
    print("%2d %9.1f | %6.0f %6.0f | %6.0f %6.0f %6.0f %6.0f %6.0f | %.1f" % (ch, st0[ch]["carrfreq"], pp[ch, 0, 0], pp[ch, 0, 1], pp[ch, 1, 0], pp[ch, 1, 1],
          pp[ch, 1, 3], pp[ch, 1, 5], pp[ch, 1, 6], pp[ch, 1, 4] * E))
print("max code loop %.0f  max carrier loop %.0f  median carrier %.0f" % (pp[:, 0, 0].max(), pp[:, 1, 0].max(), np.median(pp[:, 1, 0])))
eng.close()
