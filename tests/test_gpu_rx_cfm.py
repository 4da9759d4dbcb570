"""The correlation monitor inside the receiver schedule (-m gpu): the clean and the multipath recording of
tests/cfm_cases.py (seed cc.GPU_SEED) from a cold start, pushed in chunks of 0.25 s with one step each.

Bars.  Exact: after every step gnsscorr_rx_cfm_status equals the restated rules (tests/cfm_restate.py) run over that
step's own fetched rows with the state carried, every double as bytes; an engine with the monitor on fetches, step by
step, the bytes an engine that never switched it on fetches.  Verdicts: those tests/test_cfm_host.py finds on the oracle."""
import numpy as np
import pytest

import cfm_cases as cc
import cfm_restate as cr

pytestmark = pytest.mark.gpu
PRM = cr.prm(**cc.prm())


def _engine(gc, poison=None):
    eng = gc.Engine(0)
    if poison is not None:
        eng.debug_poison(poison)
    eng.timing(True)
    eng.ring_create(1, 2, 2 * cc.CHUNK)
    eng.set_channels(cc.channels(gc))
    eng.loop_set([eng.loop_state(i, 0.0) for i in range(cc.NCH)])
    eng.rx_start(cc.RETRY_MS)
    return eng


def _step(eng, sig, k, fetch=True):
    eng.ring_push_raw(1, sig[k * cc.CHUNK:(k + 1) * cc.CHUNK], cc.CHUNK)
    eng.rx_step(cc.MAX_PERIODS)
    if not fetch:
        return None
    II, QQ, ns = eng.trk_fetch()
    log, ndone = eng.trk_fetch_log()
    return dict(status=eng.rx_status(), II=II, QQ=QQ, ns=ns, log=log, ndone=ndone, cfm=eng.rx_cfm_status(),
                loop=[bytes(l) for l in eng.loop_get()])


def _run(gc, sig, on, prm=None, poison=None, fetch=True, nchunk=cc.NCHUNK):
    """The pushes and steps on one engine, the monitor on for the channels `on`: (history, final states, launches)."""
    eng = _engine(gc, poison)
    try:
        for i in on:
            eng.rx_cfm_set(cc.prm() if prm is None else prm, ch0=i, nch=1)
        hist = [_step(eng, sig, k, fetch) for k in range(nchunk)]
        return hist, eng.rx_cfm_status(), eng.timing_read("rx_cfm")[1]
    finally:
        eng.close()


def _restated(hist, p, on, st=None):
    """The restated monitor over each step's fetched rows, the state carried; asserts the device's states on the way
    and returns the final states and every window's event per channel."""
    st = [cr.zero_state() for _ in range(cc.NCH)] if st is None else st
    events = [[] for _ in range(cc.NCH)]
    for k, h in enumerate(hist):
        for i in range(cc.NCH):
            nd = int(h["ndone"][i])
            if i in on and nd > 0:
                cr.run(st[i], p, cc.RATE, cc.CORRN, h["II"][i], h["QQ"][i], h["log"]["flagsync"][i], h["log"]["navbit"][i], nd,
                       int(h["status"][i]["cnt"]) - nd, events=events[i])
            assert cr.same(st[i], h["cfm"][i]) == [], (k, i, cr.same(st[i], h["cfm"][i])[:4])
    return st, events


@pytest.fixture(scope="module")
def sigs(gc, synth):
    return {kind: cc.signal(gc, synth, cc.GPU_SEED, kind) for kind in cc.KINDS}


@pytest.fixture(scope="module")
def runs(gc, sigs):
    return dict(clean=_run(gc, sigs["clean"], range(cc.NCH)), off=_run(gc, sigs["clean"], []),
                multipath=_run(gc, sigs["multipath"], range(cc.NCH)))


def test_clean_recording_states_and_verdicts(gc, runs):
    hist, final, launches = runs["clean"]
    st, events = _restated(hist, PRM, range(cc.NCH))
    assert launches == cc.NCHUNK                                        # one launch per step: a channel tracks in every one
    for i in range(cc.NCH):
        assert cr.same(st[i], final[i]) == []
        assert (st[i]["windows"], st[i]["alarms"], st[i]["alarm"], st[i]["nbad"]) == (8, 0, 0, 0), (i, st[i])
        assert not any(e[5] for e in events[i]) and st[i]["bits"] == cc.SKIP_BITS + 8 * cc.KBITS + st[i]["k"]
        assert all(h["status"][i]["state"] == gc.CH_TRACK for h in hist)


def test_multipath_recording_alarms_on_prn23_only(gc, runs):
    hist, final, _ = runs["multipath"]
    st, events = _restated(hist, PRM, range(cc.NCH))
    assert (st[0]["windows"], st[0]["alarms"], st[0]["alarm"]) == (8, 0, 0) and not any(e[5] for e in events[0])
    ev = events[cc.MP_CH]
    assert [e[7] for e in ev] == [0] + [1] * 7 and all(e[6] == 1 for e in ev)   # rises at the second counted window and stays
    m = st[cc.MP_CH]
    assert (m["windows"], m["alarms"], m["alarm"], m["nbad"], m["worst_pair"]) == (8, 7, 1, 8, 1)
    ratio = np.mean([e[3] for e in ev], axis=0)
    assert 1.28 < ratio[0] < 1.295 and 0.28 < ratio[1] < 0.29 and max(np.abs(e[2]).max() for e in ev) < cc.DTOL
    assert cr.same(m, final[cc.MP_CH]) == []


def test_monitor_on_changes_nothing_the_engine_computes(gc, runs):
    """Log, II / QQ, sample counts, loop states and rx_status of every step: the bytes of an engine that never switched
    the monitor on, which times no rx_cfm launch and reports zero states."""
    (on, _, _), (off, final_off, n_off) = runs["clean"], runs["off"]
    assert n_off == 0 and final_off.tobytes() == bytes(final_off.nbytes)
    for k, (a, b) in enumerate(zip(on, off)):
        assert b["cfm"].tobytes() == bytes(b["cfm"].nbytes)
        assert a["status"] == b["status"] and a["loop"] == b["loop"], k
        assert np.array_equal(a["ndone"], b["ndone"]) and a["log"].tobytes() == b["log"].tobytes(), k
        for f in ("II", "QQ", "ns"):
            assert a[f].tobytes() == b[f].tobytes(), (k, f)


def test_monitor_for_one_channel_on_a_poisoned_engine(gc, sigs, runs):
    """The monitor on for channel 1 alone, on an engine whose every device allocation is poisoned, without a fetch
    between the steps: channel 0's state stays zero, channel 1's is the one of the engine with both on."""
    _, final, launches = _run(gc, sigs["clean"], [1], poison=0xA5, fetch=False)
    assert launches == cc.NCHUNK
    assert final[0].tobytes() == bytes(final[0].nbytes)
    assert final[1].tobytes() == runs["clean"][1][1].tobytes() and final[1]["windows"] == 8


def test_reacquisition_restart_and_housekeeping(gc, sigs):
    sig = sigs["clean"]
    p = cc.prm(skip_bits=0, kbits=5)                                     # windows from bit synchronisation on
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 2 * cc.CHUNK)
        eng.set_channels(cc.channels(gc))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(cc.NCH)])
        with pytest.raises(gc.GnsscorrError, match="rx_start"):
            eng.rx_cfm_set(p)
        with pytest.raises(gc.GnsscorrError, match="rx_start"):
            eng.rx_cfm_status()
        eng.rx_start(cc.RETRY_MS)
        st = eng.rx_cfm_status()                                         # never on: zeros
        assert st.tobytes() == bytes(st.nbytes)
        for bad, word in ((dict(p, kbits=4097), "kbits"), (dict(p, skip_bits=-1), "skip_bits"), (dict(p, nbad=0), "nbad"),
                          (dict(p, npair=3), "npair"), (dict(p, dtol=float("nan")), "dtol"), (dict(p, rtol=0.0), "rtol"),
                          (dict(p, dref=(0.0, float("inf"))), "dref"), (dict(p, rref=(float("nan"),)), "rref")):
            with pytest.raises(gc.GnsscorrError, match=word):
                eng.rx_cfm_set(bad)
        with pytest.raises(gc.GnsscorrError, match="channels"):
            eng.rx_cfm_set(p, ch0=1, nch=2)
        st = eng.rx_cfm_status()
        assert st.tobytes() == bytes(st.nbytes)
        eng.timing(True)
        eng.rx_cfm_set(p)
        # to 3.5 s: both channels are synchronised (cnt 2039) and have closed windows
        hist = [_step(eng, sig, k) for k in range(14)]
        rp = cr.prm(**p)
        st, _ = _restated(hist, rp, range(cc.NCH))
        assert all(s["windows"] >= 10 and s["alarms"] >= 1 for s in st) and eng.timing_read("rx_cfm")[1] == 14
        # channel 0 back to SEARCH: re-acquired in the next step, its cnt restarts at 0 and with it the monitor's state
        eng.rx_set(0, gc.CH_SEARCH)
        more = [_step(eng, sig, k) for k in range(14, 18)]
        assert more[0]["status"][0]["state"] == gc.CH_TRACK and more[0]["status"][0]["attempts"] == 2
        assert int(more[0]["status"][0]["cnt"]) == int(more[0]["ndone"][0]) > 0
        st, _ = _restated(more, rp, range(cc.NCH), st=st)
        now = more[-1]["cfm"]
        assert now[0].tobytes() == bytes(now[0].nbytes) and st[1]["windows"] >= 14      # not synchronised again yet: all zero
        # set between steps zeroes the named channels' states and no others; NULL switches off
        eng.rx_cfm_set(None, ch0=1, nch=1)
        st1 = eng.rx_cfm_status()
        assert st1[1].tobytes() == bytes(st1[1].nbytes)
        n = eng.timing_read("rx_cfm")[1]
        h = _step(eng, sig, 18)
        assert eng.timing_read("rx_cfm")[1] == n + 1 and h["cfm"][1].tobytes() == bytes(h["cfm"][1].nbytes)
        eng.rx_cfm_set(None)
        _step(eng, sig, 19)
        assert eng.timing_read("rx_cfm")[1] == n + 1                     # off for every channel: no launch
        # gnsscorr_rx_start leaves it off for all, the states zero
        eng.rx_cfm_set(p)
        eng.rx_start(cc.RETRY_MS)
        st = eng.rx_cfm_status()
        assert st.tobytes() == bytes(st.nbytes)
        _step(eng, sig, 20)
        assert eng.timing_read("rx_cfm")[1] == n + 1
        # so does gnsscorr_set_channels, which ends the schedule
        eng.rx_cfm_set(p)
        eng.set_channels(cc.channels(gc))
        with pytest.raises(gc.GnsscorrError, match="rx_start"):
            eng.rx_cfm_set(p)
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(cc.NCH)])
        eng.rx_start(cc.RETRY_MS)
        st = eng.rx_cfm_status()
        assert st.tobytes() == bytes(st.nbytes)
        _step(eng, sig, 21)
        assert eng.timing_read("rx_cfm")[1] == n + 1 and eng.rx_cfm_status().tobytes() == bytes(st.nbytes)
    finally:
        eng.close()
