"""GLONASS G1 from a cold start through the receiver schedule (-m gpu), on the recording of tests/g1_if_cases.py:
gnsscorr_rx_start, the recording pushed in chunks of one second with one gnsscorr_rx_step behind each, the rows of
every step replayed by gnsscorr_g1frame_replay with the cnt0 of the step's status.  The channel on frequency number +1
goes SEARCH -> TRACK in the first step and ends with flagdec and the sent time; a second channel on frequency number -1,
which nothing is sent on, stays in SEARCH and its frame state stays zero.

The search of the first step ends at the first second of the recording, and the hand-over starts cnt at 0 there: the
symbol edge is looked for from period 2001 on and found in the fourth second, in the row g1_if_cases.predict_sync gives
for the code period the tracker began in.  The time marks of strings 6 and 7 have gone by by then: the strings read are
3, 4, 5, 1, 2, just enough, and the time is merged at string 2 as in the preset runs.  Where the tracker begins is the
search's business (tests/test_gpu_rx*.py hold it to the oracle's); here every row is placed by its own buffloc, which
the code loop keeps within a sample or two of the code epoch (its error is a small fraction of a chip of four
samples)."""
import numpy as np
import pytest

import g1_if_cases as gic
import g1_restate as gr

pytestmark = pytest.mark.gpu

CHUNK = 1000 * gic.NSAMP                        # one second per push
MAX_PERIODS = 1100                              # a step's catch-up: the chunk and the search's look-back
ABSENT = -1                                     # frequency number of the channel that finds nothing


@pytest.fixture(scope="module")
def steps(gc, synth):
    sig = gic.signal(gc, synth, "phase0.7")
    n = sig.shape[0]
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 2 * CHUNK)
        eng.set_channels([gic.channel(gc), gic.channel(gc, ABSENT)])
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(2)])
        eng.rx_start(0)
        hist = []
        for a in range(0, n, CHUNK):
            m = min(CHUNK, n - a)
            eng.ring_push_raw(1, sig[a:a + m], m)
            eng.rx_step(MAX_PERIODS)
            log, ndone = eng.trk_fetch_log()
            hist.append(dict(wp=eng.ring_wrpos(1), status=eng.rx_status(), log=log, ndone=ndone, lapped=eng.trk_loop_lapped()))
        return hist
    finally:
        eng.close()


def test_cold_start_to_the_time_of_week(gc, steps):
    T, S = gc.CH_TRACK, gc.CH_SEARCH
    assert [h["status"][0]["state"] for h in steps] == [T] * len(steps) and steps[0]["status"][0]["attempts"] == 1
    acq = steps[0]["status"][0]["acq"]
    assert acq["flagacq"] == 1 and acq["acqfreq"] == gic.ACQFREQ
    assert all(h["lapped"] == 0 for h in steps)
    st, rep, total = gc.G1FrameState(), gr.G1Replay(), 0
    found = None
    for k, h in enumerate(steps):
        nd = int(h["ndone"][0])
        cnt0 = int(h["status"][0]["cnt"]) - nd
        assert cnt0 == total and nd > 0, k                                      # the steps' rows follow one another
        rows = h["log"][0][:nd]
        gc.g1frame_replay(st, rows, cnt0)
        rep.run_log(rows["navbit"], rows["buffloc"], cnt0)
        assert gr.state_fields(st) == rep.fields(), k
        total += nd
        if found is None and st.flagdec:
            found = k
        elif found is None:
            assert st.firstsftow == 0.0 and st.tow_gpst == 0.0
    # the code period of the recording that row 0 holds, and from it and the sent symbols alone: the row of the symbol
    # edge, the first symbol decided, the marks that are still to come -- strings 3, 4, 5, 1, 2 -- and their rows
    b0 = int(steps[0]["log"][0][0]["buffloc"])
    p0 = gic.P0 + round((b0 - gic.B0) / gic.NSAMP)
    assert abs(b0 - (gic.B0 + (p0 - gic.P0) * gic.NSAMP)) <= 2 and acq["buffloc"] == b0
    sync_row, synci = gic.predict_sync(gic.sent()[0], 0, p0)
    flagsync = np.concatenate([h["log"][0][:int(h["ndone"][0])]["flagsync"] for h in steps])
    assert int(np.argmax(flagsync != 0)) == sync_row and np.all(flagsync[sync_row:] == 1)
    first_symbol = (p0 + sync_row + gic.RATE - 1) // gic.RATE
    strings = [j for j in range(len(gic.NUMBERS)) if 200 * j + 170 >= first_symbol]
    assert [gic.NUMBERS[j] for j in strings] == [3, 4, 5, 1, 2]
    assert [m[0] for m in rep.marks] == [gic.RATE * (200 * j + 199) + gic.RATE - 1 - p0 for j in strings]
    assert len({pol for _, pol in rep.marks}) == 1 and st.polarity == rep.marks[0][1]
    assert found == len(steps) - 2              # (the last push is the recording's last two code periods)
    assert (st.flagsyncf, st.flagtow, st.flagdec, st.id, st.ephcnt, st.s1cnt) == (1, 1, 1, 2, 5, 2)
    assert (st.week, st.firstsftow, st.tow_gpst) == (gic.WEEK, gic.FIRSTSFTOW, gic.FIRSTSFTOW)
    assert (st.slot, st.nt, st.n4, list(st.tk)) == (gic.SLOT, gic.NT, gic.N4, [gic.TK[0] - 3, gic.TK[1], 30 * gic.TK[2]])
    # the row of firstsfcnt is the last period of the last sent symbol
    assert st.firstsfcnt == rep.marks[-1][0] and abs(int(st.firstsf) - (gic.B0 + (gic.NPER - 1) * gic.NSAMP)) <= 2
    print("acquired in step 0 at %.1f Hz; marks at cnt %s, polarity %d; flagdec in step %d of %d, firstsftow %.1f" %
          (acq["acqfreq"], [m[0] for m in rep.marks], st.polarity, found, len(steps), st.firstsftow))

    # the channel nothing is sent to: searched again and again, never tracked, nothing to replay
    absent = gc.G1FrameState()
    for h in steps:
        s = h["status"][1]
        assert s["state"] == S and s["acq"]["flagacq"] == 0 and h["ndone"][1] == 0
        gc.g1frame_replay(absent, h["log"][1], int(s["cnt"]))
    assert steps[-1]["status"][1]["attempts"] >= 2 and bytes(absent) == bytes(gc.G1FrameState())
