"""Bit synchronisation by symbol energy inside the receiver schedule (-m gpu): the scenario of tests/bsync_cases.py from
a cold start with the detector on for every channel, a control engine with it off, an engine with it on for one channel
only, PRN 133 of tests/lock_sbas_cases.py with the lock monitor beside it, and the housekeeping of the entry points.

Bars.  Exact: after every step the detector's states equal the restated rules (tests/bsync_restate.py) over that step's
fetched prompt sums and flagsync, the state carried; the preset appears in the loop state behind the deciding step and in
the rows from the next step's first period on.  Against the oracle: the rows of every step, the oracle poked with the
same flagsync / synci at the same step boundary, at the bars of tests/test_gpu_loop.py -- integers bit for bit, filter
outputs to 1e-12 with the oracle continuing from the device's values."""
import ctypes as C

import numpy as np
import pytest

import bsync_cases as bc
import bsync_restate as br
import lock_sbas_cases as ls
import rx_cases as rc
from test_gpu_loop import _adopt

pytestmark = pytest.mark.gpu
NCH = len(bc.PRNS)
A, B, CC, ABSENT = 0, 1, 2, 3


def _steps(gc, eng, sig, chunk, nchunk, max_periods, first=0):
    hist = []
    for k in range(first, nchunk):
        eng.ring_push_raw(1, sig[k * chunk:(k + 1) * chunk], chunk)
        eng.rx_step(max_periods)
        II, QQ, ns = eng.trk_fetch()
        log, ndone = eng.trk_fetch_log()
        st, applied = eng.rx_bsync_status()
        loops = eng.loop_get()
        hist.append(dict(wp=eng.ring_wrpos(1), status=eng.rx_status(), II=II, QQ=QQ, ns=ns, log=log, ndone=ndone, bsync=st,
                         applied=applied, loop=[(l.flagsync, l.synci) for l in loops]))
    return hist


def _run(gc, sig, on):
    """The scenario's pushes and steps on one engine, the detector on for the channels `on`; (history, launches timed)."""
    eng = gc.Engine(0)
    try:
        eng.timing(True)
        eng.ring_create(1, 2, 2 * bc.CHUNK)
        eng.set_channels(bc.channels(gc))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(NCH)])
        eng.rx_start(bc.RETRY_MS)
        for i in on:
            eng.rx_bsync_set(bc.PRM, ch0=i, nch=1)
        hist = _steps(gc, eng, sig, bc.CHUNK, bc.NCHUNK, bc.MAX_PERIODS)
        return hist, eng.timing_read("rx_bsync")[1]
    finally:
        eng.close()


@pytest.fixture(scope="module")
def sig(gc, synth):
    return bc.signal(gc, synth)


@pytest.fixture(scope="module")
def runs(gc, sig):
    return dict(all=_run(gc, sig, range(NCH)), off=_run(gc, sig, []), only_c=_run(gc, sig, [CC]))


def _restated(hist, prm, rates, on):
    """The restated detector over each step's fetched outputs, the state carried: per step the states (zero where the
    detector is off); asserts the device's states on the way (exact)."""
    st = [br.zero_state() for _ in rates]
    out = []
    for k, h in enumerate(hist):
        for i in range(len(rates)):
            nd = int(h["ndone"][i])
            if i in on and nd > 0:
                br.run(st[i], prm, rates[i], h["II"][i, :, 0], h["QQ"][i, :, 0], h["log"]["flagsync"][i], nd,
                       int(h["status"][i]["cnt"]) - nd)
            assert br.same(st[i], h["bsync"][i]) == [], (k, i, st[i], br.from_struct(h["bsync"][i]))
        out.append([br.copy_state(s) for s in st])
    return out


def test_cold_start_states_presets_and_rows_against_the_oracle(gc, orc, sig, runs):
    hist, launches = runs["all"]
    assert [h["wp"] for h in hist] == bc.step_wrpos()
    states = _restated(hist, bc.PRM, [bc.RATE] * NCH, range(NCH))
    assert launches == bc.NCHUNK                                    # one launch per step: a channel tracks in every one
    L = orc.lib()
    for i in (A, B, CC):
        decided = [k for k in range(bc.NCHUNK) if states[k][i]["done"] == 1]
        kd = decided[0]
        st = states[kd][i]
        ring = orc.make_ring(sig, sig.shape[0], 0)
        o = orc.make_chan(bc.PRNS[i], dtype=2, f_sf=bc.F_SF, f_if=0.0, **bc.TAPS)
        loc, _ = rc.oracle_search(orc, o, ring, bc.CHUNK)
        a = hist[0]["status"][i]["acq"]
        assert o.flagacq == 1 == a["flagacq"] and a["buffloc"] == loc and a["acqfreq"] == o.acq.acqfreq
        p0 = bc.code_period(i, loc)
        truth = bc.true_synci(i, p0)
        print("%s: decided in step %d at cnt %d, synci %d (true %d), ratio %.1f" % (bc.NAMES[i], kd, st["decided_cnt"], st["synci"],
                                                                                   truth, st["ratio_last"]))
        assert p0 == bc.P0[i] and (kd, st["synci"], st["decided_cnt"], st["tests"]) == (3, truth, 718, 1)
        assert st["ratio_last"] >= 1.1 * bc.GATE
        b = C.c_uint64(loc)
        bits, cnts = [], []
        for k, h in enumerate(hist):
            # the preset: in the loop state behind the deciding step, in the rows from the next step on
            assert int(h["applied"][i]) == (1 if k >= kd else 0), (i, k)
            assert h["loop"][i] == ((1, truth) if k >= kd else (0, 0)), (i, k, h["loop"][i])
            assert h["status"][i]["state"] == gc.CH_TRACK
            if k == kd + 1:
                assert o.flagsync == 0
                o.flagsync, o.synci = 1, truth                      # the same poke at the same step boundary
            ring.wrpos = h["wp"]
            II, QQ, ns, log, nd = h["II"][i], h["QQ"][i], h["ns"][i], h["log"][i], int(h["ndone"][i])
            cnt0 = int(o.cnt)
            e = 0
            while e < bc.MAX_PERIODS and L.orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(b)):
                where = (bc.PRNS[i], k, e)
                assert ns[e] == o.currnsamp and log[e]["currnsamp"] == o.currnsamp, where
                assert np.array_equal(II[e], np.ctypeslib.as_array(o.II)[:5]), where
                assert np.array_equal(QQ[e], np.ctypeslib.as_array(o.QQ)[:5]), where
                assert log[e]["flagloopfilter"] == o.flagloopfilter, where
                assert log[e]["remcode"] == o.remcode and log[e]["remcarr"] == o.remcarr, where
                _adopt(o, log[e], where, tol=1e-12)
                e += 1
            assert nd == e and h["status"][i]["cnt"] == o.cnt == cnt0 + e, (i, k, nd, e)
            assert np.all(log["flagsync"][:nd] == (1 if k > kd else 0)), (i, k)
            j = np.flatnonzero(log["navbit"][:nd])
            bits += [int(x) for x in log["navbit"][j]]
            cnts += [cnt0 + int(x) for x in j]
        # the decided bits are the bits sent, up to one polarity, from the preset to the end
        sent = bc.sent_bits(i, p0, cnts)
        ok = sum(int(x == y) for x, y in zip(bits, sent))
        assert len(bits) >= 98 and cnts[0] < 800 and ok in (0, len(bits)), (i, len(bits), ok)
    # the absent PRN is never acquired, so never tracked and never preset
    for k, h in enumerate(hist):
        assert h["status"][ABSENT]["state"] == gc.CH_SEARCH and h["ndone"][ABSENT] == 0 and h["applied"][ABSENT] == 0
        assert h["bsync"][ABSENT].tobytes() == bytes(h["bsync"][ABSENT].nbytes)


def test_control_engine_and_an_engine_with_the_detector_elsewhere(gc, runs):
    """The detector off: no rx_bsync launch is timed, nothing is preset, and A synchronises where the reference's rule
    does on the oracle (tests/test_bsync_host.py): at cnt 2020 with synci 0, ten periods off.  With the detector on for
    C alone, every fetch of A, B and the absent channel is bit-identical to the control's."""
    (off, n_off), (only_c, n_c), (full, _) = runs["off"], runs["only_c"], runs["all"]
    assert n_off == 0 and n_c == bc.NCHUNK
    _restated(only_c, bc.PRM, [bc.RATE] * NCH, [CC])
    for k, (a, b) in enumerate(zip(off, only_c)):
        assert not np.any(a["applied"]) and a["bsync"].tobytes() == bytes(a["bsync"].nbytes)
        for i in (A, B, ABSENT):
            assert a["ndone"][i] == b["ndone"][i] and a["status"][i] == b["status"][i], (k, i)
            assert a["log"][i].tobytes() == b["log"][i].tobytes(), (k, i)
            for f in ("II", "QQ", "ns"):
                assert a[f][i].tobytes() == b[f][i].tobytes(), (k, i, f)
            assert a["loop"][i] == b["loop"][i] and b["applied"][i] == 0
    assert [int(h["applied"][CC]) for h in only_c] == [0] * 3 + [1] * (bc.NCHUNK - 3)
    # up to and including the deciding step the detector changes nothing for its own channel either
    for k in range(4):
        for i in range(NCH):
            assert off[k]["log"][i].tobytes() == full[k]["log"][i].tobytes() and off[k]["II"][i].tobytes() == full[k]["II"][i].tobytes()

    def sync_of(hist, i):
        for h in hist:
            nd = int(h["ndone"][i])
            fs = h["log"]["flagsync"][i][:nd]
            if fs.any():
                return int(h["status"][i]["cnt"]) - nd + int(np.argmax(fs != 0)), h["loop"][i][1]
        return None

    assert sync_of(off, A) == (2020, 0) and bc.true_synci(A) == 10
    assert sync_of(off, B) == (2030, 10) and sync_of(off, CC) is None
    assert sync_of(full, A) == sync_of(full, B) == sync_of(full, CC) == (760, 10)


def test_sbas_prn133_is_preset_on_the_right_edge_and_kept(gc, synth):
    """tests/lock_sbas_cases.py with the lock monitor on as in tests/test_gpu_rx_lock_sbas.py, where PRN 133's first
    hand-over synchronises on the wrong symbol edge, looks like noise to the monitor and is sent back to SEARCH: with
    the detector on for the two SBAS channels it is preset on the right edge behind the step that holds cnt 400 and
    tracks to the end."""
    sig = ls.signal(gc, synth)
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 2 * ls.CHUNK)
        eng.set_channels(ls.channels(gc))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(3)])
        eng.rx_start(ls.RETRY_MS)
        for i in range(3):
            eng.rx_lock_set(ls.PRM[i], ch0=i, nch=1)
        eng.rx_bsync_set(bc.SBAS_PRM, ch0=0, nch=2)
        hist = _steps(gc, eng, sig, ls.CHUNK, ls.NCHUNK, ls.MAX_PERIODS)
        lock, losses = eng.rx_lock_status()
    finally:
        eng.close()
    states = _restated(hist, bc.SBAS_PRM, ls.RATES, [0, 1])
    for i in (0, 1):
        loc = hist[0]["status"][i]["acq"]["buffloc"]
        truth = br.layout_synci(ls.code_period(i, loc), 0, 2)
        st = states[-1][i]
        assert (st["done"], st["synci"], st["decided_cnt"], st["tests"]) == (1, truth, 400, 1), (i, st)
        assert st["ratio_last"] >= 1.1 * bc.SBAS_PRM["gate"]
        kd = [k for k in range(ls.NCHUNK) if states[k][i]["done"] == 1][0]
        assert kd == 2 and [int(h["applied"][i]) for h in hist[:kd + 3]] == [0] * kd + [1] * 3
        assert all(h["loop"][i] == (1, truth) for h in hist[kd:kd + 3]) and hist[-1]["applied"][1] == 1
    assert not ls.predict(1, hist[0]["status"][1]["acq"]["buffloc"])[2]         # (the reference's rule would take the wrong edge)
    assert all(h["status"][1]["state"] == gc.CH_TRACK and h["status"][1]["attempts"] == 1 for h in hist)
    assert losses[1] == 0 and lock[1]["lost"] == 0 and lock[1]["windows"] >= 50 and lock[1]["mu_last"] > ls.MU_MIN
    assert all(h["status"][2]["state"] == gc.CH_TRACK for h in hist) and losses[2] == 0 and not np.any(hist[-1]["applied"][2:])


def test_housekeeping_of_the_entry_points(gc, sig):
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 2 * bc.CHUNK)
        eng.set_channels(bc.channels(gc))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(NCH)])
        with pytest.raises(gc.GnsscorrError, match="rx_start"):
            eng.rx_bsync_set(bc.PRM)
        with pytest.raises(gc.GnsscorrError, match="rx_start"):
            eng.rx_bsync_status()
        eng.rx_start(bc.RETRY_MS)
        st, applied = eng.rx_bsync_status()                         # never on: zeros
        assert st.tobytes() == bytes(st.nbytes) and not np.any(applied)
        for bad, word in ((dict(bc.PRM, start_cnt=-1), "start_cnt"), (dict(bc.PRM, nsym=-2), "nsym"), (dict(bc.PRM, nsym=101), "nsym"),
                          (dict(bc.PRM, nsym_max=4097), "nsym_max"), (dict(bc.PRM, gate=0.5), "gate")):
            with pytest.raises(gc.GnsscorrError, match=word):
                eng.rx_bsync_set(bad)
        with pytest.raises(gc.GnsscorrError, match="channels"):
            eng.rx_bsync_set(bc.PRM, ch0=3, nch=2)
        eng.timing(True)
        eng.rx_bsync_set(bc.PRM)
        eng.rx_bsync_set(None, ch0=B, nch=1)                        # off again for B
        hist = _steps(gc, eng, sig, bc.CHUNK, 3, bc.MAX_PERIODS)
        st = hist[-1]["bsync"]
        assert st[A]["armed"] == 1 and st[CC]["armed"] == 1 and st[A]["n"] >= 10 and eng.timing_read("rx_bsync")[1] == 3
        assert st[B].tobytes() == bytes(st[B].nbytes)
        # set between steps zeroes the named channels' states and no others
        eng.rx_bsync_set(dict(bc.PRM, start_cnt=300), ch0=A, nch=1)
        now, _ = eng.rx_bsync_status()
        assert now[A].tobytes() == bytes(now[A].nbytes) and now[CC].tobytes() == st[CC].tobytes()
        h = _steps(gc, eng, sig, bc.CHUNK, 4, bc.MAX_PERIODS, first=3)[0]
        assert h["bsync"][A]["a0"] == int(h["status"][A]["cnt"]) - int(h["ndone"][A]) and h["bsync"][CC]["done"] == 1 and h["applied"][CC] == 1
        # gnsscorr_rx_start switches it off for all and starts the applied counts over
        eng.rx_start(bc.RETRY_MS)
        n = eng.timing_read("rx_bsync")[1]
        _, applied = eng.rx_bsync_status()
        assert not np.any(applied)
        _steps(gc, eng, sig, bc.CHUNK, 5, bc.MAX_PERIODS, first=4)
        assert eng.timing_read("rx_bsync")[1] == n == 4
        # so does gnsscorr_set_channels, which ends the schedule
        eng.set_channels(bc.channels(gc))
        with pytest.raises(gc.GnsscorrError, match="rx_start"):
            eng.rx_bsync_set(bc.PRM)
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(NCH)])
        eng.rx_start(bc.RETRY_MS)
        st, applied = eng.rx_bsync_status()
        assert st.tobytes() == bytes(st.nbytes) and not np.any(applied)
    finally:
        eng.close()
