"""Three L1 C/A satellites from IF samples to observation epochs on the device (-m gpu), on the recording of
tests/sync_if_cases.py with the ring as the span: gnsscorr_trk_run_loop free-running from the bit-synchronised state,
gnsscorr_trk_fetch and gnsscorr_trk_fetch_log, gnsscorr_frame_replay and gnsscorr_obs_replay per channel, then the
gnsscorr_sync_* calls.  tests/test_sync_if_host.py shows on the oracle alone what the recording holds.

Bars: the epochs of the run cut into three calls equal those of one call bit for bit; both equal the restatement
tests/sync_restate.py applied to the device's own rows bit for bit; the epochs are the oracle chain's (the same tows with
the same satellites); every pseudorange difference is within three times the oracle chain's worst error of the
synthesiser's truth -- the device's loop differs from the oracle's by ulps of atan, so three times is room, not a second
measurement -- and every Doppler within 25 Hz."""
import numpy as np
import pytest

import sync_if_cases as sic
import sync_restate as sr

pytestmark = pytest.mark.gpu

_TRACKED = {}


def tracked(gc, synth, runs):
    """The recording tracked on the device in the calls `runs`: per call (log [3, n], II0 [3, n]).  Once per process."""
    if runs in _TRACKED:
        return _TRACKED[runs]
    sig = sic.signal(gc, synth)
    n = sig.shape[0]
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, n)
        eng.ring_push_raw(1, sig, n)
        chans = sic.channels(gc)
        assert all(c.nsamp == sic.NSAMP for c in chans)
        eng.set_channels(chans)
        eng.trk_set_state([dict(carrfreq=sic.DOPPLERS[i], codefreq=c.crate, remcode=0.0, remcarr=0.0, buffloc=sic.b0(i))
                           for i, c in enumerate(chans)])
        eng.loop_set([eng.loop_state(i, sic.DOPPLERS[i], flagsync=1, synci=sic.synci(i), cnt=sic.CNT0[i]) for i in range(3)])
        calls = []
        for nrun in runs:
            eng.trk_run_loop(nrun)
            II, _, _ = eng.trk_fetch()
            log, ndone = eng.trk_fetch_log()
            assert list(ndone) == [nrun] * 3
            calls.append((log.copy(), II[:, :, 0].copy()))
        _TRACKED[runs] = calls
    finally:
        eng.close()
    return calls


def oracle_epochs(gc, orc, synth):
    pushes = []
    for i, (log, I) in enumerate(sic.oracle_run(gc, orc, synth)):
        pushes.append(sic.one_push(i, sic.replays(gc, i, sic.cut(log), I)[1]))
    return sic.full_epochs(sic.library(gc, pushes)), sic.by_epoch(sic.library(gc, pushes))


def check_epochs(gc, orc, synth, out, pushes, frames, what):
    assert sr.same_bits(out, sic.restated(pushes))
    for i, fr in enumerate(frames):
        assert (fr.flagdec, fr.sfid, fr.firstsftow, fr.firstsfcnt) == (1, sic.SFID, sic.FIRSTSFTOW, sic.CNT0[i] + sic.found_row(i))
    want, want_all = oracle_epochs(gc, orc, synth)
    eps = sic.full_epochs(out)
    assert [(tow, sorted(sat)) for tow, sat in sic.by_epoch(out)] == [(tow, sorted(sat)) for tow, sat in want_all]
    assert [k for k, _ in eps] == [k for k, _ in want] == list(range(1, sic.NROWS_AFTER + 1))
    for k, sat in eps:
        for i in range(3):
            assert sat[i]["week"] == sic.WEEK and abs(sat[i]["D"] + sic.DOPPLERS[i]) < 25.0
    oracle_worst, worst = sic.worst_range_error(want), sic.worst_range_error(eps)
    print("%s: %d epochs, worst |P_i - P_j - truth| = %.3f m (oracle chain %.3f m)" % (what, len(eps), worst, oracle_worst))
    assert worst <= 3 * oracle_worst


def test_one_run_one_push_per_channel(gc, orc, synth):
    (log, I), = tracked(gc, synth, (sic.NPER,))
    pushes, frames = [], []
    for i in range(3):
        fr, out = sic.replays(gc, i, sic.cut(log[i]), I[i])
        pushes.append(sic.one_push(i, out))
        frames.append(fr)
    check_epochs(gc, orc, synth, sic.library(gc, pushes), pushes, frames, "one run")


def test_three_runs_pushed_per_run(gc, orc, synth):
    """Runs of 700, 1300 and the remaining periods; after each run every channel's rows are replayed and pushed, with the
    frame state as it is then, and nothing is flushed until the end."""
    calls = tracked(gc, synth, sic.PIECES)
    (log1, I1), = tracked(gc, synth, (sic.NPER,))
    assert np.concatenate([c[0] for c in calls], axis=1).tobytes() == log1.tobytes()
    per = [sic.replays(gc, i, [c[0][i] for c in calls], np.concatenate([c[1][i] for c in calls])) for i in range(3)]
    pushes = [(i, *per[i][1][n]) for n in range(len(calls)) for i in range(3)]
    assert [p[1].flagdec for p in pushes] == [0] * 6 + [1] * 3
    out = sic.library(gc, pushes)
    check_epochs(gc, orc, synth, out, pushes, [fr for fr, _ in per], "three runs")
    one = [sic.one_push(i, sic.replays(gc, i, sic.cut(log1[i]), I1[i])[1]) for i in range(3)]
    assert sr.same_bits(out, sic.library(gc, one))
