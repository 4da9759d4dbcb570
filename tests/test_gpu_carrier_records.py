"""The batch planner's carrier chain on staged records (gnsscorr_plan.hip: plan4_car_wave; gnsscorr_nco.h:
gc_car_rec_make, gc_carrier_rec_step_one) on the GPU: 4 channels x 130 periods, two batches back to back (blocks of
64, 64 and 2 periods).

  * falling from remcarr -803 rad at -4321.5 Hz: the phase crosses |x| = 4096, 8192 and 16384 LUT steps inside the
    run, so some periods straddle a binade and must leave the record's one-binade step;
  * falling at -31 Hz;
  * rising at 8765.25 Hz;
  * on the 200-Hz grid from remcarr 0.

Final remcarr and every period's sums and sample count equal the oracle's sdrtracking() bit for bit, the carrier
tallies add up to the periods planned, and the per-channel counters of periods served by the records' own steps
(gnsscorr_debug_plan_rec: window step, one-binade record step) say that the new path ran: the falling channel took
the record's one-binade step in at least 90 % of its periods and left it in at least three (a period that straddles
a binade cannot pass |y| <= top), the rising channel took the window step from its records."""
import ctypes as C

import numpy as np
import pytest

NEPOCH, NBATCH = 130, 2
NS = 16368
NSAMP = NS * (NEPOCH * NBATCH + 8)
CARR = [(-4321.5, -803.0), (-31.0, -2.5), (8765.25, 1.25), (1400.0, 0.0)]


@pytest.mark.gpu
def test_carrier_records_against_oracle(gc, orc, engine):
    rng = np.random.default_rng(5150)
    data = rng.integers(-60, 61, size=(NSAMP, 2), dtype=np.int8)
    eng = engine
    eng.ring_create(1, 2, NSAMP)
    eng.ring_push_raw(1, data, NSAMP)
    chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3) for p in (3, 11, 19, 27)]
    eng.set_channels(chans)
    states = [dict(carrfreq=f, codefreq=c.crate + 0.75 * (i - 1.5), remcode=0.2 + 0.15 * i, remcarr=r, buffloc=100 + 37 * i)
              for i, (c, (f, r)) in enumerate(zip(chans, CARR))]
    eng.trk_set_state(states)
    stats = np.zeros(8, dtype=np.uint64)
    gc.lib().gnsscorr_debug_plan_stats(C.c_void_p(stats.ctypes.data), 1)
    rec = np.zeros((64, 2), dtype=np.uint64)
    assert gc.lib().gnsscorr_debug_plan_rec(C.c_void_p(rec.ctypes.data), 1) == 0
    out = []
    for _ in range(NBATCH):
        eng.trk_run(NEPOCH)
        II, QQ, ns = eng.trk_fetch()
        out.append((II.copy(), QQ.copy(), ns.copy()))
    fin = eng.trk_get_state()
    gc.lib().gnsscorr_debug_plan_stats(C.c_void_p(stats.ctypes.data), 1)
    assert gc.lib().gnsscorr_debug_plan_rec(C.c_void_p(rec.ctypes.data), 1) == 0
    ring = orc.make_ring(data, NSAMP, NSAMP)
    for i, (c, st) in enumerate(zip(chans, states)):
        o = orc.make_chan(c.prn, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3)
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
        b = st["buffloc"]
        for e in range(NEPOCH * NBATCH):
            orc.lib().orc_sdrtracking(C.byref(o), C.byref(ring), b)
            bt, et = divmod(e, NEPOCH)
            II, QQ, ns = out[bt]
            assert ns[i, et] == o.currnsamp, (i, e)
            assert np.array_equal(II[i, et], np.ctypeslib.as_array(o.II)[:5]), (i, e)
            assert np.array_equal(QQ[i, et], np.ctypeslib.as_array(o.QQ)[:5]), (i, e)
            b += o.currnsamp
        assert fin[i]["remcarr"].hex() == o.remcarr.hex(), i
        assert fin[i]["remcode"].hex() == o.remcode.hex() and int(fin[i]["buffloc"]) == b, i
    # (every trk_run also plans the batch behind the one it correlates: the tallies cover the batches run and that one)
    per_batch = len(chans) * NEPOCH
    car, code = int(stats[3]) + int(stats[4]) + int(stats[5]), int(stats[0]) + int(stats[1]) + int(stats[2])
    assert car == code == (NBATCH + 1) * per_batch, stats.tolist()
    assert int(stats[6]) == 0, stats.tolist()
    # what served the periods, per channel (P: the channel's periods planned).  The shares are those of the CPU chains of
    # tests/test_nco_carrier_rec.py, which take the same steps from the same records.
    P = NEPOCH * (car // per_batch)
    win, one = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64)
    print("record steps per channel (window, one binade):", win[:4].tolist(), one[:4].tolist(), "of", P)
    assert not rec[4:].any()
    assert 0.9 * P <= one[0] <= P - 3, (win[:4].tolist(), one[:4].tolist())       # -4321.5 Hz: three binade crossings leave the step
    assert win[1] + one[1] >= 0.9 * P and one[1] > 0, (win[:4].tolist(), one[:4].tolist())     # -31 Hz
    assert win[2] >= 0.9 * P and one[2] == 0, (win[:4].tolist(), one[:4].tolist())             # 8765.25 Hz: a rising phase is wrapped every period
    assert int(win.sum() + one.sum()) <= int(stats[3])
