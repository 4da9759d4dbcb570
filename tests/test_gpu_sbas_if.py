"""SBAS L1 from IF samples to frames on the device (-m gpu), on the signals of tests/sbas_if_cases.py: a 500 symbol/s
stream tied to the code epoch, tracked by gnsscorr_trk_run_loop from the hand-over state through the symbol
synchronisation (checksync / checkbit at rate 2), its log rows replayed by gnsscorr_sbasframe_replay and decoded by
gnsscorr_fec_run.  tests/test_sbas_if_host.py shows on the oracle alone what the signals hold.

Bars: tracking against the oracle under teacher forcing exactly as tests/test_gpu_loop.py holds it (sums, samples,
remainders, flags and decided symbols of every row bit for bit, filter outputs to 1e-12 as the mixed-receiver tests), the
nav state after every call field for field; the frame state against the plain replay of tests/fec_restate.py on the same
rows field for field, and against what the signal was built to hold; decoder rows against fec_restate.fec_rows bit for
bit."""
import numpy as np
import pytest

import fec_restate as fr
import sbas_if_cases as sic
from test_gpu_loop import _check_against_oracle
from test_gpu_loop_mixed import _check_final
from test_gpu_sbasframe import _fields, _same

pytestmark = pytest.mark.gpu

_TRACKED = {}


def tracked(gc, orc, synth, name):
    """The case tracked on the device in the calls of sic.CHUNKS, every period checked against the oracle and the nav
    state after every call: dict(c, logs: one array of TrkLog per call, log: all rows, sync: flagsync of the loop state
    after each call).  Once per process."""
    if name in _TRACKED:
        return _TRACKED[name]
    c = sic.case(name)
    sig = sic.signal(gc, synth, name)
    n = sig.shape[0]
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, n)
        eng.ring_push_raw(1, sig, n)
        ch = gc.Channel(sic.PRN, ctype=gc.CTYPE_L1SBAS, dtype=2, f_sf=sic.F_SF, f_if=0.0, **sic.TAPS)
        assert ch.nsamp == sic.NSAMP
        eng.set_channels([ch])
        eng.trk_set_state([dict(carrfreq=sic.ACQFREQ, codefreq=ch.crate, remcode=0.0, remcarr=0.0, buffloc=sic.B0)])
        eng.loop_set([eng.loop_state(0, sic.ACQFREQ, flagsync=0, synci=0, cnt=c["cnt0"])])
        o, b = sic.oracle_channel(orc, c)
        ring = orc.make_ring(sig, n, n)
        logs, sync, done = [], [], 0
        for nrun in sic.CHUNKS:
            _check_against_oracle(orc, eng, [o], ring, [b], nrun, 5, done=done, tol=1e-12)
            log, ndone = eng.trk_fetch_log()
            assert ndone[0] == nrun
            logs.append(log[0].copy())
            # flagsync, synci, biti, navcnt, swloop, swreset, swsync, bit, bitIP, the register, cnt and the sums
            lst = _check_final(eng, [o], [b], 5)
            sync.append(int(lst[0].flagsync))
            done += nrun
        assert abs(o.carrfreq - sic.DOPPLER) < 30.0
        _TRACKED[name] = dict(c=c, logs=logs, log=np.concatenate(logs), sync=sync, synci=int(o.synci))
    finally:
        eng.close()
    return _TRACKED[name]


def _decided(t):
    """(symbols, cnts, bufflocs) of the rows of the device's log that decided a symbol."""
    log, c = t["log"], t["c"]
    rows = np.flatnonzero(log["navbit"])
    return log["navbit"][rows].astype(np.int8), c["cnt0"] + rows, log["buffloc"][rows]


@pytest.mark.parametrize("name", ["right_phase0.7", "wrong_edge"])
def test_tracking_through_symbol_sync_equals_the_oracle(gc, orc, synth, name):
    """The whole run of 4013 periods in six calls, the one-period loop, checksync's shift register on signs that change
    every second period, then the two-period loop with bitIP * IP < 0 live: every row against orc_sdrthread_step, the nav
    state after every call.  And the oracle, hence the device, found the edge the sent symbols predict."""
    t = tracked(gc, orc, synth, name)
    c, log = t["c"], t["log"]
    assert len(log) == sic.NPER
    assert int(np.argmax(log["flagsync"] != 0)) == c["sync_row"] and np.all(log["flagsync"][c["sync_row"]:] == 1)
    assert t["sync"] == [0, 1, 1, 1, 1, 1] and t["synci"] == c["synci"]
    assert np.array_equal(np.flatnonzero(log["navbit"]), c["rows"])
    # before the edge the filters run every period, behind it in the row after each decided symbol's first period
    assert np.all(log["flagloopfilter"][:c["sync_row"]] == 1)
    assert set(np.unique(log["flagloopfilter"][c["sync_row"] + 2:])) == {0, 2}
    if c["right"]:
        sym, _, _ = _decided(t)
        assert np.array_equal(sym, c["polarity"] * c["sent"][c["symi"]])


@pytest.mark.parametrize("name", list(sic.CASES))
def test_replay_of_the_devices_log_finds_the_sent_frame(gc, orc, synth, engine, name):
    """gnsscorr_sbasframe_replay on the device's own rows, in one call: equal to the plain replay on the same rows, and to
    what the signal carries -- message 0 at the predicted cnt with the polarity of the carrier phase, through the flipped
    symbols in the flip case; nothing on the wrong edge."""
    t = tracked(gc, orc, synth, name)
    c, log = t["c"], t["log"]
    st = gc.SbasFrameState()
    engine.sbasframe_replay(st, log, c["cnt0"])
    sym, cnts, locs = _decided(t)
    rep = sic.replayed(sym, cnts, locs)
    _same(st, rep)
    print("%s: flagsync in row %d, firstsfcnt predicted %s, found %d (flagdec %d), polarity %d" %
          (name, int(np.argmax(log["flagsync"] != 0)), c["firstsfcnt"], st.firstsfcnt, st.flagdec, st.polarity))
    if c["right"]:
        assert (st.flagtow, st.flagsyncf, st.flagdec, st.flagpol) == (1, 1, 1, 0)
        assert st.firstsfcnt == c["firstsfcnt"] and st.firstsf == int(log["buffloc"][c["found_row"]])
        assert bytes(st.msg) == c["msg"] and st.polarity == c["polarity"]
        assert (st.id, st.tow, st.week, st.firstsftow) == (12, sic.TOW, sic.WEEK, sic.TOW)
        wrong = sym != c["polarity"] * c["clean"][c["symi"]]
        assert np.array_equal(c["symi"][wrong], c["flips"])              # the hard decisions are wrong where flipped
    else:
        assert st.flagtow == 0 and _fields(st) == fr.SbasReplay().fields()


@pytest.mark.parametrize("name", ["right_phase3.84", "wrong_edge"])
def test_replay_in_the_pieces_of_the_tracking_calls(gc, orc, synth, engine, name):
    """Each trk_run_loop call's rows with its cnt0: a call of one period, a cut between the two periods of a symbol, a cut
    right before the row of firstsfcnt.  The final state equals that of one call over all rows."""
    t = tracked(gc, orc, synth, name)
    c = t["c"]
    one = gc.SbasFrameState()
    engine.sbasframe_replay(one, t["log"], c["cnt0"])
    st, cnt = gc.SbasFrameState(), c["cnt0"]
    for rows in t["logs"]:
        if c["right"] and cnt == c["firstsfcnt"]:
            assert st.flagtow == 0                                       # (not found before its row)
        engine.sbasframe_replay(st, rows, cnt)
        cnt += len(rows)
    assert bytes(st) == bytes(one)
    _same(st, sic.replayed(*_decided(t)))
    assert (st.flagdec, st.firstsfcnt) == ((1, c["firstsfcnt"]) if c["right"] else (0, 0))


@pytest.mark.parametrize("name", ["right_flips", "wrong_edge"])
def test_decoder_windows_on_the_tracked_symbols(gc, orc, synth, engine, name):
    """gnsscorr_fec_run on the decided symbol column: every window, stride 1 -- the leading zeros of the unfilled history,
    then the tracker's symbols (flipped ones, and on the wrong edge decisions made on noise)."""
    sym, _, _ = _decided(tracked(gc, orc, synth, name))
    assert len(sym) > 1990
    got = engine.fec_run(sym, 0, len(sym))
    assert np.array_equal(got, fr.fec_rows(sym, 0, len(sym)))
    assert len(np.unique(got[0], axis=0)) > 1900
