"""Frames, observables and epochs behind every step, on the device (-m gpu): gnsscorr_rx_nav_start / _step and
gnsscorr_trk_fetch_prompt on recordings other test files synthesise -- tests/sync_if_cases.py without the schedule,
tests/g1_if_cases.py from a cold start with it, tests/lock_cases.py with the lock monitor on.  After every step the
context's driver is compared with the reference composition tests/rxnav_cases.py::Compose fed from that step's own
plain fetches (gnsscorr_trk_fetch_log, gnsscorr_trk_fetch, the status): status, frame states byte for byte, rows and
epochs, all as equalities; and gnsscorr_trk_fetch_prompt with tap 0 of gnsscorr_trk_fetch, bit for bit."""
import hashlib

import numpy as np
import pytest

import g1_if_cases as gic
import g1_restate as gr
import lock_cases as lc
import rxnav_cases as rc
import sync_if_cases as sic
import sync_restate as sr
from test_gpu_sync_if import check_epochs

pytestmark = pytest.mark.gpu

# sha256 over the fetches of rx_digest() below, taken with the library of the commit before the nav driver existed
PARENT_DIGEST = "e21fccdc22c5cfc3ae952efd2c502eb34d7f56f7a5e9090e0e8b195e81c68dfd"


def compose_for(gc, eng, outms, hold):
    """Compose with the constants gnsscorr_rx_nav_start takes: the channel table, loopms of the loop constants, the
    tracking state's remcode."""
    loops, states = eng.loop_get(), eng.trk_get_state()
    return rc.Compose(gc, [rc.chan_of(gc, ch, loopms=loops[i].loopms, oldremcode=states[i]["remcode"])
                           for i, ch in enumerate(eng.channels)], outms, hold)


def step_both(gc, eng, nav, cmp, nper, sched, where):
    """One rx_nav_step, compose fed from the step's plain fetches, everything compared; sched: the schedule is on.
    Returns (epochs, log, ndone, status)."""
    eng.rx_nav_step(nper)
    II, QQ, _ = eng.trk_fetch()
    II0, QQ0 = eng.trk_fetch_prompt()
    assert II0.tobytes() == np.ascontiguousarray(II[:, :, 0]).tobytes() and QQ0.tobytes() == np.ascontiguousarray(QQ[:, :, 0]).tobytes(), where
    log, ndone = eng.trk_fetch_log()
    if sched:
        status = eng.rx_status()
        cnt, tracking = [s["cnt"] for s in status], [int(s["state"] == gc.CH_TRACK) for s in status]
    else:
        status = None
        cnt, tracking = [l.cnt for l in eng.loop_get()], [1] * len(eng.channels)
    cmp.feed(log, II[:, :, 0], ndone, cnt, tracking, eng=eng)
    rc.assert_same(gc, nav, cmp, where)
    return rc.assert_same_epochs(nav, cmp, where), log, ndone, status


# ---- schedule off: three L1 C/A satellites ------------------------------------------------------------------------------
def test_schedule_off_three_l1ca_satellites(gc, orc, synth):
    sig = sic.signal(gc, synth)
    n = sig.shape[0]
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, n)
        eng.ring_push_raw(1, sig, n)
        chans = sic.channels(gc)
        eng.set_channels(chans)
        eng.trk_set_state([dict(carrfreq=sic.DOPPLERS[i], codefreq=c.crate, remcode=0.0, remcarr=0.0, buffloc=sic.b0(i))
                           for i, c in enumerate(chans)])
        eng.loop_set([eng.loop_state(i, sic.DOPPLERS[i], flagsync=1, synci=sic.synci(i), cnt=sic.CNT0[i]) for i in range(3)])
        eng.rx_nav_start(sic.OUTMS, 0)
        nav, cmp = eng.rx_nav(), compose_for(gc, eng, sic.OUTMS, 0)
        for k in range(3):
            nav.week(k, sic.WEEK)
            cmp.week(k, sic.WEEK)
        out = []
        for k, nper in enumerate(sic.PIECES):
            epo, _, ndone, _ = step_both(gc, eng, nav, cmp, nper, False, "piece %d" % k)
            assert list(ndone) == [nper] * 3
            out += epo
        nav.flush()
        cmp.flush()
        out += rc.assert_same_epochs(nav, cmp, "flush")
        frames = [nav.frame(k, gc.CTYPE_L1CA) for k in range(3)]
        assert [p[1].flagdec for p in cmp.pushes] == [0] * 6 + [1] * 3
        check_epochs(gc, orc, synth, out, cmp.pushes, frames, "rx_nav_step, three runs")
        cmp.close()
    finally:
        eng.close()


# ---- schedule on, cold start: GLONASS G1 -------------------------------------------------------------------------------
def test_schedule_on_g1_cold_start(gc, synth):
    CHUNK, MAX_PERIODS, OUTMS = 1000 * gic.NSAMP, 1100, 10      # as tests/test_gpu_g1_rx.py pushes and steps
    sig = gic.signal(gc, synth, "phase0.7")
    n = sig.shape[0]
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 2 * CHUNK)
        eng.set_channels([gic.channel(gc), gic.channel(gc, -1)])
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(2)])
        eng.rx_start(0)
        eng.rx_nav_start(OUTMS, 2)
        nav, cmp = eng.rx_nav(), compose_for(gc, eng, OUTMS, 2)
        out, rep, found, nsteps = [], gr.G1Replay(), None, 0
        for a in range(0, n, CHUNK):
            m = min(CHUNK, n - a)
            eng.ring_push_raw(1, sig[a:a + m], m)
            epo, log, ndone, status = step_both(gc, eng, nav, cmp, MAX_PERIODS, True, "second %d" % nsteps)
            out += epo
            nd = int(ndone[0])
            rows = log[0][:nd]
            rep.run_log(rows["navbit"], rows["buffloc"], int(status[0]["cnt"]) - nd)
            st = nav.status(2)
            if found is None and st["flagdec"][0]:
                found = nsteps
            # the absent channel is never attached and has zero state and zero resets
            assert status[1]["state"] == gc.CH_SEARCH and ndone[1] == 0
            assert (st["attached"][1], st["resets"][1], st["nrows"][1], st["flagdec"][1]) == (0, 0, 0, 0)
            assert bytes(nav.frame(1, gc.CTYPE_G1)) == bytes(gc.G1FrameState())
            nsteps += 1
        fr, st = nav.frame(0, gc.CTYPE_G1), nav.status(2)
        assert gr.state_fields(fr) == rep.fields() and found == nsteps - 2
        assert (st["flagdec"][0], st["week"][0], st["firstsftow"][0], st["id"][0]) == (1, gic.WEEK, gic.FIRSTSFTOW, 2)
        assert st["firstsfcnt"][0] == rep.marks[-1][0] and abs(int(fr.firstsf) - (gic.B0 + (gic.NPER - 1) * gic.NSAMP)) <= 2
        nav.flush()
        cmp.flush()
        out += rc.assert_same_epochs(nav, cmp, "flush")
        # epochs of one satellite on the outms grid
        assert len(out) >= 1 and all((e[0], e[1]) == (0, gic.WEEK) for e in out)
        for e in out:
            ms = (e[2] - sr.PTIMING / 1000) * 1000
            assert abs(ms - round(ms)) < 1e-3 and round(ms) % OUTMS == 0 and e[2] >= gic.FIRSTSFTOW
        print("flagdec in step %d of %d, %d epochs from tow %.3f on" % (found, nsteps, len(out), out[0][2]))
        cmp.close()
    finally:
        eng.close()


# ---- loss and re-acquisition ----------------------------------------------------------------------------------------------
_LOCK_SIG = []


def lock_signal(gc, synth):
    if not _LOCK_SIG:
        _LOCK_SIG.append(lc.signal(gc, synth))
    return _LOCK_SIG[0]


def test_loss_and_reacquisition(gc, synth):
    sig = lock_signal(gc, synth)
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 2 * lc.CHUNK)
        eng.set_channels(lc.channels(gc))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(len(lc.PRNS))])
        eng.rx_start(lc.RETRY_MS)
        for i, p in enumerate(lc.PRNS):
            eng.rx_lock_set(lc.prm_of(p), ch0=i, nch=1)
        eng.rx_nav_start(10, 2)
        nav, cmp = eng.rx_nav(), compose_for(gc, eng, 10, 2)
        T, hist, out = gc.CH_TRACK, [], []
        for k in range(lc.NCHUNK):
            eng.ring_push_raw(1, sig[k * lc.CHUNK:(k + 1) * lc.CHUNK], lc.CHUNK)
            epo, _, ndone, status = step_both(gc, eng, nav, cmp, lc.MAX_PERIODS, True, "step %d" % k)
            out += epo
            hist.append(dict(state=[s["state"] for s in status], cnt=[s["cnt"] for s in status], ndone=list(ndone), nav=nav.status(4),
                             nrows=[len(nav.rows(i)) for i in range(4)]))
        # PRN 12 (channel 1): detached and zeroed in the step whose status shows it out of TRACK
        s12 = [h["state"][1] for h in hist]
        first = s12.index(T)
        lost = next(k for k in range(first, len(hist)) if s12[k] != T)
        back = next(k for k in range(lost, len(hist)) if s12[k] == T)
        assert hist[lost - 1]["nav"]["attached"][1] == 1 and hist[lost - 1]["nav"]["nrows"][1] > 0 and hist[lost - 1]["nav"]["resets"][1] == 0
        h = hist[lost]["nav"]
        assert (h["attached"][1], h["nrows"][1], h["resets"][1], h["flagsyncf"][1], h["tow"][1]) == (0, 0, 1, 0, 0.0)
        # ... and makes rows again after its second hand-over, nrows counted from there
        assert hist[back]["cnt"][1] == hist[back]["ndone"][1] > 0
        end = hist[-1]["nav"]
        assert end["attached"][1] == 1 and end["resets"][1] == 1
        assert end["nrows"][1] == sum(h["nrows"][1] for h in hist[back:]) > 0
        # PRN 5 is never reset; PRN 30 ends detached; PRN 9 never delivers
        assert (end["resets"][0], end["attached"][0]) == (0, 1) and end["nrows"][0] == sum(h["nrows"][0] for h in hist)
        assert hist[-1]["state"][2] != T and (end["attached"][2], end["nrows"][2], end["resets"][2]) == (0, 0, 1)
        assert (end["attached"][3], end["resets"][3], end["cnt"][3]) == (0, 0, 0)
        # no epochs: the recording carries no frame
        nav.flush()
        cmp.flush()
        out += rc.assert_same_epochs(nav, cmp, "flush")
        assert out == [] and not any(end["flagdec"])
        print("PRN 12: TRACK from step %d, out of TRACK in step %d, back in step %d; rows at the end %d" % (first, lost, back, end["nrows"][1]))
        cmp.close()
    finally:
        eng.close()


# ---- SBAS beside L1 C/A: the replay that runs on the device ------------------------------------------------------------
def test_sbas_channels_beside_l1ca(gc, synth):
    """The recording of tests/lock_sbas_cases.py (SBAS PRN 120 switched off at 6.3 s, SBAS PRN 133 first on the wrong
    symbol edge, L1 C/A PRN 12), the monitor on: the driver's switch on the code type sends two channels through
    gnsscorr_sbasframe_replay with the context.  PRN 120 has its time from the message of type 12 without aid, so its
    rows become epochs until it is lost; PRN 12 has no week and makes none."""
    import lock_sbas_cases as ls
    sig = ls.signal(gc, synth)
    nch = len(ls.PRNS)
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 2 * ls.CHUNK)
        eng.set_channels(ls.channels(gc))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(nch)])
        eng.rx_start(ls.RETRY_MS)
        for i in range(nch):
            eng.rx_lock_set(ls.PRM[i], ch0=i, nch=1)
        eng.rx_nav_start(10, 2)
        nav, cmp = eng.rx_nav(), compose_for(gc, eng, 10, 2)
        assert [c["loopms"] for c in cmp.cfg] == [2, 2, 10]
        out, decoded, states = [], None, []
        for k in range(ls.NCHUNK):
            eng.ring_push_raw(1, sig[k * ls.CHUNK:(k + 1) * ls.CHUNK], ls.CHUNK)
            epo, _, _, status = step_both(gc, eng, nav, cmp, ls.MAX_PERIODS, True, "step %d" % k)
            out += epo
            states.append([s["state"] for s in status])
            st = nav.status(nch)
            if decoded is None and st["flagdec"][0]:
                decoded = k
                assert (st["week"][0], st["firstsftow"][0], st["attached"][0]) == (ls.WEEK, ls.TOW, 1)
        nav.flush()
        cmp.flush()
        out += rc.assert_same_epochs(nav, cmp, "flush")
        end = nav.status(nch)
        lost = next(k for k in range(ls.NCHUNK) if states[k][0] != gc.CH_TRACK)
        assert decoded is not None and decoded < lost and ls.T_OFF < (lost + 1) * 0.25
        assert (end["attached"][0], end["resets"][0], end["nrows"][0], end["flagdec"][0]) == (0, 1, 0, 0)
        assert (end["attached"][1], end["resets"][1]) == (1, 1) and (end["attached"][2], end["resets"][2], end["week"][2]) == (1, 0, 0)
        assert len(out) >= 10 and all((e[0], e[1]) == (0, ls.WEEK) and e[2] >= ls.TOW for e in out)
        print("PRN 120: frame in step %d, out of TRACK in step %d, %d epochs" % (decoded, lost, len(out)))
        cmp.close()
    finally:
        eng.close()


# ---- lifecycle -------------------------------------------------------------------------------------------------------------
def test_lifecycle(gc, synth):
    sig = lock_signal(gc, synth)
    L = gc.lib()
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 2 * lc.CHUNK)
        eng.set_channels(lc.channels(gc))
        assert L.gnsscorr_rx_nav_start(eng.h, 10, 0) == gc.ESTATE           # no loop constants yet
        loops = [eng.loop_state(i, 0.0) for i in range(len(lc.PRNS))]
        eng.loop_set(loops)
        assert L.gnsscorr_rx_nav_step(eng.h, 10) == gc.ESTATE and eng.rx_nav() is None      # before rx_nav_start
        assert L.gnsscorr_rx_nav_stop(eng.h) == gc.ESTATE
        eng.rx_nav_start(10, 0)
        assert eng.rx_nav() is not None
        eng.set_channels(lc.channels(gc))                                   # switches it off
        assert L.gnsscorr_rx_nav_step(eng.h, 10) == gc.ESTATE and eng.rx_nav() is None
        eng.loop_set(loops)
        eng.rx_nav_start(10, 0)
        eng.rx_start(lc.RETRY_MS)                                           # a later rx_start does, too
        assert L.gnsscorr_rx_nav_step(eng.h, 10) == gc.ESTATE and eng.rx_nav() is None
        assert "rx_nav_start" in L.gnsscorr_last_error().decode()
        eng.rx_nav_start(10, 0)                                             # the schedule has not stepped: fine
        eng.rx_nav_stop()
        assert eng.rx_nav() is None
        eng.ring_push_raw(1, sig[:lc.CHUNK], lc.CHUNK)
        eng.rx_step(lc.MAX_PERIODS)
        assert all(s["attempts"] == 1 for s in eng.rx_status())
        assert L.gnsscorr_rx_nav_start(eng.h, 10, 0) == gc.ESTATE and eng.rx_nav() is None      # after a step of the schedule
        eng.rx_start(lc.RETRY_MS)
        eng.rx_nav_start(10, 0)
        eng.ring_create(1, 2, 2 * lc.CHUNK)                                 # re-creating the channels' ring: schedule and driver off
        assert L.gnsscorr_rx_nav_step(eng.h, 10) == gc.ESTATE and eng.rx_nav() is None
    finally:
        eng.close()


def rx_digest(gc, sig, nsteps=6):
    """The first steps of the tests/lock_cases.py scenario without the monitor and without the nav driver: sha256 over
    every step's log, ndone, II, QQ and status counters."""
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 2 * lc.CHUNK)
        eng.set_channels(lc.channels(gc))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(len(lc.PRNS))])
        eng.rx_start(lc.RETRY_MS)
        h = hashlib.sha256()
        for k in range(nsteps):
            eng.ring_push_raw(1, sig[k * lc.CHUNK:(k + 1) * lc.CHUNK], lc.CHUNK)
            eng.rx_step(lc.MAX_PERIODS)
            II, QQ, ns = eng.trk_fetch()
            log, ndone = eng.trk_fetch_log()
            for a in (log, ndone, II, QQ, ns):
                h.update(np.ascontiguousarray(a).tobytes())
            h.update(repr([(s["state"], s["attempts"], s["next_try"], s["cnt"], s["acq"]["buffloc"]) for s in eng.rx_status()]).encode())
        return h.hexdigest()
    finally:
        eng.close()


def test_rx_step_without_the_driver_is_the_parent_commits(gc, synth):
    got = rx_digest(gc, lock_signal(gc, synth))
    print("rx_step digest %s (parent commit %s)" % (got, PARENT_DIGEST))
    assert got == PARENT_DIGEST
