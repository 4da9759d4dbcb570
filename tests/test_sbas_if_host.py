"""The signals of tests/sbas_if_cases.py on the CPU oracle alone (no GPU): orc_sdrthread_step from the hand-over state
with cnt preset just below 2000, free-running, then the plain replay of fec_restate.py on the symbols the oracle decided.
This pins what the signals hold -- the row in which the symbol edge is found, which edge it is, every decided symbol,
where the frame is found and what it says -- before tests/test_gpu_sbas_if.py asks the device for the same."""
import ctypes as C

import numpy as np
import pytest

import fec_restate as fr
import sbas_if_cases as sic

_RUNS = {}


def oracle_run(gc, orc, synth, name):
    """dict(flagsync, navbit, buffloc, I: [NPER] columns of the oracle's rows, synci, o: the channel after the run)."""
    if name not in _RUNS:
        c = sic.case(name)
        sig = sic.signal(gc, synth, name)
        ring = orc.make_ring(sig, sig.shape[0], sig.shape[0])
        o, b = sic.oracle_channel(orc, c)
        L = orc.lib()
        fs, nb, loc, I = (np.zeros(sic.NPER, t) for t in (np.int32, np.int32, np.uint64, np.float64))
        for e in range(sic.NPER):
            loc[e] = b.value
            assert L.orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(b)) == 1
            fs[e], nb[e], I[e] = o.flagsync, (o.bit if (o.flagsync and o.swsync) else 0), o.II[0]
        _RUNS[name] = dict(flagsync=fs, navbit=nb, buffloc=loc, I=I, synci=int(o.synci), o=o)
    return _RUNS[name]


def test_case_geometry():
    """What the case file derives, on the sent symbols alone."""
    right, wrong, flip = sic.case("right_phase0.7"), sic.case("wrong_edge"), sic.case("right_flips")
    assert (sic.P0, sic.B0, sic.NPER, sic.FOUND_ROW, sum(sic.CHUNKS)) == (1, 3691, 4013, 3036, sic.NPER)
    assert (right["sync_row"], right["synci"], right["right"], right["firstsfcnt"]) == (12, 0, True, 5026)
    # cnt0 = 1991: rows 10 and 11 (cnt 2001, 2002) are the second period of symbol 5 and the first of symbol 6, which
    # were sent with the same sign
    assert right["sent"][5] == right["sent"][6]
    assert (wrong["sync_row"], wrong["synci"], wrong["right"], wrong["firstsfcnt"]) == (11, 0, False, None)
    # cuts: a call of one period, between the two periods of a symbol on either edge, right before the row of firstsfcnt
    cuts = np.cumsum(sic.CHUNKS)
    assert 1 in sic.CHUNKS and 1500 in cuts and 1501 in cuts and sic.FOUND_ROW in cuts
    assert 1500 in right["rows"] and 1501 in wrong["rows"]          # the closing row is the first row of the next call
    # week as the message holds it, and the flips
    assert sic.WEEK - 1024 < 1024
    idx = flip["flips"]
    assert idx.size >= 10 and idx.min() >= sic.LEAD + 64 and idx.max() < sic.LEAD + 1512 - 64
    assert np.array_equal(np.flatnonzero(flip["sent"] != flip["clean"]), idx)
    # few enough that the decoder alone still returns messages 0 and 1 (the frame path reads bits 0..257; the window ends
    # inside message 3, so the chainback from state 0 may miss its last bits with or without flips)
    bits = [b for m in sic.messages() for b in m]
    win = flip["sent"][sic.LEAD:sic.LEAD + fr.WIN]
    assert np.array_equal(fr.viterbi27(win, fr.NDEC)[:500], np.array(bits[:500]))
    hard = (win.astype(int) != flip["clean"][sic.LEAD:sic.LEAD + fr.WIN]).sum()
    assert hard == idx.size


@pytest.mark.parametrize("name", list(sic.CASES))
def test_oracle_finds_the_edge_the_symbols_and_the_frame(gc, orc, synth, name):
    c = sic.case(name)
    r = oracle_run(gc, orc, synth, name)
    # the symbol edge: flagsync rises in the predicted row and stays, synci as predicted
    assert int(np.argmax(r["flagsync"] != 0)) == c["sync_row"] and np.all(r["flagsync"][c["sync_row"]:] == 1)
    assert not np.any(r["flagsync"][:c["sync_row"]]) and r["synci"] == c["synci"]
    # a symbol is decided in exactly the predicted rows
    assert np.array_equal(np.flatnonzero(r["navbit"]), c["rows"])
    assert abs(r["o"].carrfreq - sic.DOPPLER) < 30.0
    dec = r["navbit"][c["rows"]]
    rep = sic.replayed(dec, c["cnts"], r["buffloc"][c["rows"]])
    if c["right"]:
        # every decided symbol is the transmitted one, flipped ones included, times the sign the carrier loop settled on
        assert np.array_equal(dec, c["polarity"] * c["sent"][c["symi"]])
        assert np.array_equal(dec != c["polarity"] * c["clean"][c["symi"]], np.isin(c["symi"], c["flips"]))
        assert (rep.flagtow, rep.flagsyncf, rep.flagdec, rep.flagpol) == (1, 1, 1, 0)
        assert rep.firstsfcnt == c["firstsfcnt"] and rep.firstsf == int(r["buffloc"][c["found_row"]])
        assert (rep.polarity, rep.msg, rep.id) == (c["polarity"], c["msg"], 12)
        assert (rep.tow, rep.week, rep.firstsftow, rep.tow_gpst) == (sic.TOW, sic.WEEK, sic.TOW, sic.TOW)
    else:
        # every decision adds the second period of one symbol and the first of the next: where the two differ it is made on
        # noise, and the Costas loop, fed the same sums, slips half a cycle every few tens of symbols (a right edge
        # correlates with the sent stream at +-1; here neither neighbour's stream is in the decisions)
        a, b = c["sent"][c["symi"] - 1], c["sent"][c["symi"]]
        assert 0.4 < (a == b).mean() < 0.6
        assert abs(float((dec * a).mean())) < 0.5 and abs(float((dec * b).mean())) < 0.5
        assert rep.fields() == fr.SbasReplay().fields() and rep.flagtow == 0 and rep.ndecodes == len(dec)
