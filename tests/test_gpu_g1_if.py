"""GLONASS G1 from IF samples to the time of week on the device (-m gpu), on the recording of tests/g1_if_cases.py:
gnsscorr_trk_run_loop free-running from the hand-over state through the bit synchronisation (checksync's vote branch at
rate 10), the `navbit` column of its log through gnsscorr_g1frame_replay, and the frame state into gnsscorr_obs_replay.
tests/test_g1_if_host.py shows on the oracle alone what the recording holds.

Bars: every decided symbol and the row it is decided in equal the free-running oracle's (the two loops differ by ulps of
the filters' atan, so the filter columns are not compared here: tests/test_gpu_loop.py and test_gpu_loop_mixed.py hold
those under teacher forcing, G1 channels included); the library's frame state equals the restatement's on the same rows
field for field, and what the signal was built to carry; everything about the frame is exact."""
import numpy as np
import pytest

import g1_if_cases as gic
import g1_restate as gr

pytestmark = pytest.mark.gpu

EXTRA = 2                                       # rows behind the last sent symbol that the recording still holds
_TRACKED = {}


def tracked(gc, synth, name, chunks):
    """The case tracked on the device in the calls `chunks`: dict(c, logs: one array of TrkLog per call, log: all rows,
    I: the prompt sum of every row).  Once per process and (name, chunks)."""
    key = (name, tuple(chunks))
    if key in _TRACKED:
        return _TRACKED[key]
    c = gic.case(name)
    sig = gic.signal(gc, synth, name)
    n = sig.shape[0]
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, n)
        eng.ring_push_raw(1, sig, n)
        ch = gic.channel(gc)
        assert (ch.nsamp, ch.foffset) == (gic.NSAMP, gic.FOFFSET)
        eng.set_channels([ch])
        eng.trk_set_state([dict(carrfreq=gic.ACQFREQ, codefreq=ch.crate, remcode=0.0, remcarr=0.0, buffloc=gic.B0)])
        eng.loop_set([eng.loop_state(0, gic.ACQFREQ, flagsync=0, synci=0, cnt=c["cnt0"])])
        logs, I = [], []
        for nrun in chunks:
            eng.trk_run_loop(nrun)
            II, _, _ = eng.trk_fetch()
            log, ndone = eng.trk_fetch_log()
            assert ndone[0] == nrun
            logs.append(log[0].copy())
            I.append(II[0, :, 0].copy())
        lst = eng.loop_get()[0]
        assert lst.cnt == c["cnt0"] + sum(chunks) and abs(lst.acqfreq + lst.carrNco - gic.FOFFSET - gic.DOPPLER) < 30.0
        _TRACKED[key] = dict(c=c, logs=logs, log=np.concatenate(logs), I=np.concatenate(I))
    finally:
        eng.close()
    return _TRACKED[key]


def _built_to_hold(st, c, log):
    assert (st.flagsyncf, st.flagtow, st.flagdec, st.polarity) == (1, 1, 1, c["polarity"])
    assert (st.firstsfcnt, st.firstsf) == (c["cnt0"] + gic.FOUND_ROW, int(log["buffloc"][gic.FOUND_ROW]))
    assert (st.week, st.firstsftow, st.tow_gpst) == (gic.WEEK, gic.FIRSTSFTOW, gic.FIRSTSFTOW)
    assert (st.slot, st.nt, st.n4, list(st.tk)) == (gic.SLOT, gic.NT, gic.N4, [gic.TK[0] - 3, gic.TK[1], 30 * gic.TK[2]])
    assert (st.id, st.ephcnt, st.s1cnt) == (2, 5, 2)


@pytest.mark.parametrize("name", list(gic.CASES))
def test_device_symbols_equal_the_oracles_and_carry_the_frame(gc, orc, synth, name):
    """One call over all rows: the navbit column equals the oracle's, row for row; the replay of the device's log equals
    the restatement's field for field and finds the seven marks, the polarity of the phase and the sent time."""
    t = tracked(gc, synth, name, (gic.NPER + EXTRA,))
    c, log = t["c"], t["log"][:gic.NPER]
    r = gic.oracle_run(gc, orc, synth, name)
    assert np.array_equal(log["navbit"], r["navbit"]) and np.array_equal(log["flagsync"], r["flagsync"])
    assert int(np.argmax(log["flagsync"] != 0)) == c["sync_row"]
    assert np.array_equal(log["navbit"][c["rows"]], c["polarity"] * c["sent"][c["symi"]])
    st = gc.G1FrameState()
    gc.g1frame_replay(st, log, c["cnt0"])
    rep = gic.replayed(log["navbit"], log["buffloc"])
    assert gr.state_fields(st) == rep.fields()
    assert rep.marks == [(c["cnt0"] + row, c["polarity"]) for row in gic.MARK_ROWS]
    _built_to_hold(st, c, log)
    print("%s: flagsync in row %d, marks at cnt %s, polarity %d, week %d firstsftow %.1f" %
          (name, c["sync_row"], [m[0] for m in rep.marks], st.polarity, st.week, st.firstsftow))


def test_tracking_calls_cut_inside_a_symbol_and_around_a_mark_row(gc, synth):
    """The same run in the calls of gic.CHUNKS -- a cut inside a symbol, one row before the row of a time mark, one row
    after it -- each call's rows replayed with its cnt0: the rows, and the final frame state, are those of one call."""
    name = "phase3.84"
    one = tracked(gc, synth, name, (gic.NPER + EXTRA,))
    cut = tracked(gc, synth, name, gic.CHUNKS)
    c = one["c"]
    assert cut["log"].tobytes() == one["log"][:gic.NPER].tobytes()
    whole = gc.G1FrameState()
    gc.g1frame_replay(whole, one["log"][:gic.NPER], c["cnt0"])
    st, rep, cnt = gc.G1FrameState(), gr.G1Replay(), c["cnt0"]
    for rows in cut["logs"]:
        gc.g1frame_replay(st, rows, cnt)
        rep.run_log(rows["navbit"], rows["buffloc"], cnt)
        assert gr.state_fields(st) == rep.fields()
        cnt += len(rows)
        if cnt - c["cnt0"] == gic.MARK_ROWS[2] + 1:     # string 3's mark, found in the two-row call: dropped, no time yet
            assert (st.firstsfcnt, st.id, st.ephcnt, st.flagtow) == (cnt - 1, 3, 1, 0)
    assert bytes(st) == bytes(whole)
    _built_to_hold(st, c, cut["log"])


@pytest.mark.parametrize("name", list(gic.CASES))
def test_observables_take_their_time_from_the_g1_frame(gc, synth, name):
    """gnsscorr_obs_replay fed flagsyncf / polarity / firstsfcnt / firstsftow from the G1 state, as a caller's loop does
    (INTEGRATION.md 4c): the frame state after each piece goes into the observables' state before that piece's rows.  The
    rows from flagdec on carry tow = firstsftow + (cnt - firstsfcnt) * ctime, the sent time; flagdec rises in the row of
    the last sent symbol, which is a row of observables (the prm2 update of a 10 ms symbol falls on its last period)."""
    t = tracked(gc, synth, name, (gic.NPER + EXTRA,))
    c, log, I = t["c"], t["log"], t["I"]
    ch = gic.channel(gc)
    obs, st = gc.ObsState(), gc.G1FrameState()
    obs.f_sf, obs.f_if, obs.foffset, obs.ctime, obs.loopms = gic.F_SF, 0.0, gic.FOFFSET, ch.ctime, 10
    out, a = [], 0
    for n in (gic.FOUND_ROW, len(log) - gic.FOUND_ROW):
        rows = log[a:a + n]
        gc.g1frame_replay(st, rows, c["cnt0"] + a)
        if st.flagdec:
            obs.flagsyncf, obs.polarity, obs.firstsfcnt, obs.firstsftow = st.flagsyncf, st.polarity, st.firstsfcnt, st.firstsftow
        out.append(gc.obs_replay(obs, rows, I[a:a + n], cnt0=c["cnt0"] + a))
        a += n
    assert st.flagdec == 1 and len(out[0]) > 1300 and np.all(out[0]["tow"] == out[0]["cntout"] * ch.ctime)      # (no frame yet)
    after = out[1]
    assert len(after) == 1 and int(after[0]["cntout"]) == st.firstsfcnt == c["cnt0"] + gic.FOUND_ROW
    for r in after:
        assert r["tow"] == st.firstsftow + (int(r["cntout"]) - st.firstsfcnt) * ch.ctime
        sent = gic.TOW1 + (gic.P0 + int(r["cntout"]) - c["cnt0"] + 1 - 2000 * 5) * 1e-3      # the end of that row's code period
        assert r["tow"] == sent == gic.FIRSTSFTOW
    assert int(after[0]["codei"]) == st.firstsf and obs.flagpolarityadd == 1
