"""The lock monitor inside the receiver schedule (-m gpu): the scenario of tests/lock_cases.py -- PRN 5 always on, PRN 12
off from 3 s to 5 s, PRN 30 off after 1 s, PRN 9 absent -- on one engine with the monitor on and on a control engine with
it off.  The detector's verdicts are checked against its restatement over the very outputs the device tracked
(tests/lock_restate.py), the schedule against the rule applied to those verdicts.  tests/test_lock_host.py shows on the
oracle alone what the scenario decides."""
import numpy as np
import pytest

import lock_cases as lc
import lock_restate as lr

pytestmark = pytest.mark.gpu


TIMED_STEPS = 4                              # the last steps run with gnsscorr_timing on


def _run(gc, sig, monitor):
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 2 * lc.CHUNK)
        eng.set_channels(lc.channels(gc))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(len(lc.PRNS))])
        eng.rx_start(lc.RETRY_MS)
        if monitor:
            for i, p in enumerate(lc.PRNS):
                eng.rx_lock_set(lc.prm_of(p), ch0=i, nch=1)
        hist = []
        for k in range(lc.NCHUNK):
            if k == lc.NCHUNK - TIMED_STEPS:
                eng.timing(True)
            eng.ring_push_raw(1, sig[k * lc.CHUNK:(k + 1) * lc.CHUNK], lc.CHUNK)
            eng.rx_step(lc.MAX_PERIODS)
            II, QQ, _ = eng.trk_fetch()
            log, ndone = eng.trk_fetch_log()
            lock, losses = eng.rx_lock_status()
            hist.append(dict(wp=eng.ring_wrpos(1), status=eng.rx_status(), I=II[:, :, 0].copy(), Q=QQ[:, :, 0].copy(), log=log,
                             ndone=ndone, lock=lock, losses=losses, II=II, QQ=QQ))
        return hist, dict(rx_lock=eng.timing_read("rx_lock"), tail=eng.timing_read("trk_step_tail"))
    finally:
        eng.close()


@pytest.fixture(scope="module")
def runs(gc, synth):
    sig = lc.signal(gc, synth)
    on, on_timers = _run(gc, sig, True)
    off, off_timers = _run(gc, sig, False)
    return dict(on=on, off=off, on_timers=on_timers, off_timers=off_timers)


@pytest.fixture(scope="module")
def verdicts(runs):
    """The restated detector over each step's fetched outputs, the state carried: per step and channel the state and
    whether the step declared the channel lost.  Asserts the device's states on the way."""
    st = [lr.zero_state() for _ in lc.PRNS]
    out = []
    for k, h in enumerate(runs["on"]):
        words = []
        for i, p in enumerate(lc.PRNS):
            nd = int(h["ndone"][i])
            cnt0 = int(h["status"][i]["cnt"]) - nd
            ev = []
            lr.run(st[i], lc.prm_of(p), lc.RATE, h["I"][i], h["Q"][i], h["log"]["flagsync"][i], h["log"]["navbit"][i], nd, cnt0, events=ev)
            assert lr.same(st[i], h["lock"][i]) == [], (k, p, st[i], lr.from_struct(h["lock"][i]))
            words.append(int(any(e[0] == "lost" for e in ev)))
        out.append(dict(words=words, st=[dict(s) for s in st]))
    return out


def test_lock_status_equals_restatement_after_every_step(runs, verdicts):
    assert len(verdicts) == lc.NCHUNK and [h["wp"] for h in runs["on"]] == lc.step_wrpos()
    # the monitor saw synchronised bits and windows, not only zeros
    last = verdicts[-1]["st"]
    assert last[0]["windows"] >= 15 and last[0]["mu_last"] > 16.0 and last[0]["lost"] == 0
    assert last[1]["windows"] >= 2 and last[3] == lr.zero_state()


def test_status_history_follows_the_verdicts_and_the_schedule_rule(gc, runs, verdicts):
    for i, p in enumerate(lc.PRNS):
        ch = dict(state=gc.CH_SEARCH, next_try=lc.FIRST_TRY, attempts=0, losses=0)
        word = 0
        for k, h in enumerate(runs["on"]):
            s = h["status"][i]

            def search(wp):
                assert s["acq_wrpos"] == wp, (p, k, s)                  # the device searched in this very step
                return bool(s["acq"]["flagacq"])

            before = dict(ch)
            lc.schedule_step(ch, h["wp"], word, search)
            where = (p, k, s, ch)
            assert (s["state"], s["attempts"], int(h["losses"][i])) == (ch["state"], ch["attempts"], ch["losses"]), where
            if ch["state"] == gc.CH_SEARCH:
                assert s["next_try"] == ch["next_try"] and h["ndone"][i] == 0, where
            if word and before["state"] == gc.CH_TRACK:                 # loss in step k - 1: SEARCH and one more attempt now
                assert ch["attempts"] == before["attempts"] + 1 and ch["losses"] == before["losses"] + 1, where
                if ch["state"] == gc.CH_SEARCH:
                    assert ch["next_try"] == h["wp"] + lc.RETRY_SAMPLES, where     # the pause, on the sample clock
            word = verdicts[k]["words"][i]


def test_scenario_outcomes(gc, runs, verdicts):
    on = runs["on"]
    states = lambda i: [h["status"][i]["state"] for h in on]
    T, S = gc.CH_TRACK, gc.CH_SEARCH
    # PRN 5: TRACK throughout, never lost
    assert states(0) == [T] * lc.NCHUNK and all(h["losses"][0] == 0 for h in on)
    # PRN 12: lost once by the power rule, searched in the gap, paused, acquired again after the signal is back
    lost_steps = [k for k, v in enumerate(verdicts) if v["words"][1]]
    assert len(lost_steps) == 1
    kl = lost_steps[0]
    st = verdicts[kl]["st"][1]
    assert (st["lost"], st["reason"]) == (1, 2)
    h = on[kl]
    row = st["lost_cnt"] - (int(h["status"][1]["cnt"]) - int(h["ndone"][1]))
    t_lost = float(h["log"]["buffloc"][1][row]) / lc.F_SF
    limit = (lc.PRM["nbad"] + 1) * lc.PRM["kbits"] * lc.RATE * 1e-3
    assert lc.T_OFF_12 < t_lost <= lc.T_OFF_12 + limit, t_lost
    s12 = states(1)
    back = s12.index(T, kl + 1)
    assert s12 == [T] * (kl + 1) + [S] * (back - kl - 1) + [T] * (lc.NCHUNK - back)
    assert on[back]["wp"] / lc.F_SF > lc.T_ON_12 and on[back]["status"][1]["cnt"] == on[back]["ndone"][1] > 0   # cnt restarted
    assert on[back]["status"][1]["attempts"] == 3 and on[kl + 1]["status"][1]["acq"]["flagacq"] == 0
    assert all(h["losses"][1] == (1 if k > kl else 0) for k, h in enumerate(on))
    fin = verdicts[-1]["st"][1]
    assert fin["lost"] == 0 and fin["windows"] >= 2 and fin["mu_last"] > 16.0      # the new run synchronised and is healthy
    # PRN 30: acquired, never synchronised, lost by the time limit, SEARCH to the end
    l30 = [k for k, v in enumerate(verdicts) if v["words"][2]]
    assert len(l30) == 1
    st = verdicts[l30[0]]["st"][2]
    assert (st["lost"], st["reason"], st["lost_cnt"]) == (1, 1, lc.PRM["sync_periods"] - 1)
    assert states(2) == [T] * (l30[0] + 1) + [S] * (lc.NCHUNK - l30[0] - 1) and on[-1]["losses"][2] == 1
    # PRN 9: never acquired
    assert states(3) == [S] * lc.NCHUNK and on[-1]["losses"][3] == 0 and on[-1]["status"][3]["attempts"] == 6


def test_control_engine_without_the_monitor(gc, runs):
    """The monitor off: PRN 12 and PRN 30 track noise to the end as before, no rx_lock launch is timed; and the
    monitor disturbs nothing: PRN 5's outputs are bit-identical in the two engines in every step."""
    on, off = runs["on"], runs["off"]
    for i in (0, 1, 2):
        assert [h["status"][i]["state"] for h in off] == [gc.CH_TRACK] * lc.NCHUNK, i
    assert all(not np.any(h["losses"]) for h in off)
    assert all(h["lock"].tobytes() == bytes(h["lock"].nbytes) for h in off)
    assert runs["off_timers"]["rx_lock"] == (0.0, 0) and runs["off_timers"]["tail"][1] > TIMED_STEPS
    assert runs["on_timers"]["rx_lock"][1] == TIMED_STEPS and runs["on_timers"]["rx_lock"][0] > 0.0    # one launch per step
    for k, (a, b) in enumerate(zip(on, off)):
        assert a["ndone"][0] == b["ndone"][0] > 0, k
        assert a["log"][0].tobytes() == b["log"][0].tobytes(), k
        assert a["II"][0].tobytes() == b["II"][0].tobytes() and a["QQ"][0].tobytes() == b["QQ"][0].tobytes(), k
        assert a["status"][0] == b["status"][0], k


def test_lock_set_refuses_bad_values_and_needs_a_schedule(gc, engine):
    engine.ring_create(1, 2, 2 * lc.CHUNK)
    engine.set_channels(lc.channels(gc, [5, 12]))
    engine.loop_set([engine.loop_state(i, 0.0) for i in range(2)])
    with pytest.raises(gc.GnsscorrError, match="rx_start"):
        engine.rx_lock_set(lc.PRM)
    with pytest.raises(gc.GnsscorrError, match="rx_start"):
        engine.rx_lock_status()
    engine.rx_start()
    for bad, word in ((dict(kbits=4097), "kbits"), (dict(nbad=0), "nbad"), (dict(sync_periods=-1), "sync_periods"),
                      (dict(mu_min=0.0), "mu_min"), (dict(mu_min=20.5), "mu_min")):
        with pytest.raises(gc.GnsscorrError, match=word):
            engine.rx_lock_set(dict(lc.PRM, **bad))
    with pytest.raises(gc.GnsscorrError):
        engine.rx_lock_set(lc.PRM, ch0=1, nch=2)
    engine.rx_lock_set(lc.PRM)
    engine.rx_lock_set(None, ch0=0, nch=1)                              # off again for channel 0
    engine.rx_lock_set(dict(lc.PRM, kbits=0), ch0=1, nch=1)             # kbits 0: off as well
    st, losses = engine.rx_lock_status()
    assert st.tobytes() == bytes(st.nbytes) and not np.any(losses)
