"""The signal of tests/g1_if_cases.py on the CPU oracle alone (no GPU): orc_sdrthread_step from the hand-over state with
cnt preset just below 2000, free-running over the 14 000 code periods, then gnsscorr_g1frame_replay and the plain replay
of g1_restate.py on the log the oracle wrote.  This pins what the signal holds -- the row in which the symbol edge is
found, every decided symbol, the rows of the seven time marks, what strings 3, 4, 5, 1, 2 say and the time they give --
before tests/test_gpu_g1_if.py asks the device for the same."""
import numpy as np
import pytest

import g1_if_cases as gic
import g1_restate as gr
import g1_strings as gs


def oracle_log(gc, r):
    log = np.zeros(gic.NPER, dtype=np.dtype(gc.TrkLog))
    log["navbit"], log["buffloc"], log["flagsync"] = r["navbit"], r["buffloc"], r["flagsync"]
    return log


def test_case_geometry():
    """What the case file derives, on the sent symbols alone."""
    c = gic.case("phase0.7")
    assert (gic.P0, gic.B0, gic.NPER, gic.CODEPHASE, sum(gic.CHUNKS)) == (1, 1640, 13999, 101.80078125, gic.NPER)
    assert (gic.CODEPHASE + gic.B0 * 511 / 2048) == 511.0                    # row 0 begins on a code epoch
    assert gic.MARK_ROWS == [1998, 3998, 5998, 7998, 9998, 11998, 13998] and gic.ACQFREQ == 562500.0 - 800.0
    assert (c["sync_row"], c["synci"]) == (689, 8) and c["rows"][0] == 698 and c["symi"][0] == 69
    assert c["symi"][0] < 170                   # the symbol edge is there before the first time mark begins
    assert (gic.NT, gic.N4, gic.WEEK, gic.FIRSTSFTOW) == (1233, 7, 2262, 300352.0)
    # the cuts: inside a symbol, one row before a mark row, one row after it
    cuts = np.cumsum(gic.CHUNKS)
    assert list(cuts[:3]) == [1004, 5997, 5999] and not np.isin([1004, 5997, 5999], c["rows"]).any() and 5998 in c["rows"]
    # the sent stream on its own carries the frame: symbols straight into the restatement
    rep = gr.G1Replay().run(c["sent"], np.arange(gic.NSYM) * 10, np.zeros(gic.NSYM, np.int64))
    assert (rep.flagdec, rep.firstsftow, rep.week, rep.slot, rep.s1cnt) == (1, gic.FIRSTSFTOW, gic.WEEK, gic.SLOT, 2)
    assert [m[0] for m in rep.marks] == [2000 * j + 1990 for j in range(7)]


@pytest.mark.parametrize("name", list(gic.CASES))
def test_oracle_finds_the_symbols_the_marks_and_the_time(gc, orc, synth, name):
    c = gic.case(name)
    r = gic.oracle_run(gc, orc, synth, name)
    # bit synchronisation rises in the predicted row and stays, synci as predicted
    assert int(np.argmax(r["flagsync"] != 0)) == c["sync_row"] and np.all(r["flagsync"][c["sync_row"]:] == 1)
    assert not np.any(r["flagsync"][:c["sync_row"]]) and r["synci"] == c["synci"]
    assert abs(r["carrfreq"] - gic.FOFFSET - gic.DOPPLER) < 30.0
    # a symbol is decided in exactly the predicted rows, and every one is the sent symbol times the sign the carrier loop
    # settled on
    assert np.array_equal(np.flatnonzero(r["navbit"]), c["rows"])
    assert np.array_equal(r["navbit"][c["rows"]], c["polarity"] * c["sent"][c["symi"]])
    # the replay of that log: library == restatement, field for field
    log = oracle_log(gc, r)
    st = gc.G1FrameState()
    gc.g1frame_replay(st, log, c["cnt0"])
    rep = gic.replayed(r["navbit"], r["buffloc"])
    assert gr.state_fields(st) == rep.fields()
    # ... and what the signal was built to hold: the seven marks at the predicted rows with the polarity of the phase
    assert rep.marks == [(c["cnt0"] + row, c["polarity"]) for row in gic.MARK_ROWS]
    assert (st.flagsyncf, st.flagtow, st.flagdec, st.polarity) == (1, 1, 1, c["polarity"])
    assert (st.firstsfcnt, st.firstsf) == (c["cnt0"] + gic.FOUND_ROW, int(r["buffloc"][gic.FOUND_ROW]))
    assert (st.week, st.firstsftow, st.tow_gpst) == (gic.WEEK, gic.FIRSTSFTOW, gic.FIRSTSFTOW)
    assert (st.slot, st.nt, st.n4, list(st.tk)) == (gic.SLOT, gic.NT, gic.N4, [gic.TK[0] - 3, gic.TK[1], 30 * gic.TK[2]])
    assert (st.id, st.ephcnt, st.s1cnt, st.iode, st.update) == (2, 5, 2, gic.IODE, 1) and bytes(st.str) == gs.packed(c["bits"][-1])


def test_replay_of_the_oracle_log_in_pieces(gc, orc, synth):
    """The cuts of gic.CHUNKS, each piece with its cnt0: the same final state; no time before string 2's mark row."""
    c = gic.case("phase3.84")
    log = oracle_log(gc, gic.oracle_run(gc, orc, synth, "phase3.84"))
    one = gc.G1FrameState()
    gc.g1frame_replay(one, log, c["cnt0"])
    st, a = gc.G1FrameState(), 0
    for n in gic.CHUNKS:
        gc.g1frame_replay(st, log[a:a + n], c["cnt0"] + a)
        a += n
        if a <= gic.FOUND_ROW:
            assert (st.flagtow, st.flagdec, st.tow_gpst) == (0, 0, 0.0)
    assert a == gic.NPER and bytes(st) == bytes(one) and st.flagdec == 1
