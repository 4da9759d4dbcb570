"""The lock monitor at rate 2 inside the receiver schedule (-m gpu): the scenario of tests/lock_sbas_cases.py -- SBAS
PRN 120 on the right symbol edge and switched off at 6.3 s, SBAS PRN 133 on the wrong edge, L1 C/A PRN 12 beside them, so
that every monitor launch holds bit lengths of 2 and 20 periods in one workgroup -- on one engine with the monitor on and
on a control engine with it off.

Two bars.  Exact: after every step the monitor's state equals the restated detector (tests/lock_restate.py) over that
step's fetched prompt sums, flagsync and navbit, the state carried; status, attempts and losses follow
lock_cases.schedule_step applied to those verdicts; the frame state of gnsscorr_sbasframe_replay over the steps' rows
equals the plain replay of tests/fec_restate.py on the same rows.  Within one step: the step in which the device loses a
channel against the step in which the free-running oracle loses it (tests/test_lock_host.py shows what the oracle
decides); the two loops differ by ulps of the filters' atan, so their window means are not the same numbers."""
import numpy as np
import pytest

import fec_restate as fr
import lock_cases as lc
import lock_restate as lr
import lock_sbas_cases as ls
import sbas_if_cases as sic
from test_gpu_sbasframe import _fields, _same

pytestmark = pytest.mark.gpu

NCH = len(ls.PRNS)


def _run(gc, sig, monitor):
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 2 * ls.CHUNK)
        eng.set_channels(ls.channels(gc))
        loops = [eng.loop_state(i, 0.0) for i in range(NCH)]
        assert [l.rate for l in loops] == ls.RATES
        eng.loop_set(loops)
        eng.rx_start(ls.RETRY_MS)
        if monitor:
            for i in range(NCH):
                eng.rx_lock_set(ls.PRM[i], ch0=i, nch=1)
        hist = []
        for k in range(ls.NCHUNK):
            eng.ring_push_raw(1, sig[k * ls.CHUNK:(k + 1) * ls.CHUNK], ls.CHUNK)
            eng.rx_step(ls.MAX_PERIODS)
            II, QQ, _ = eng.trk_fetch()
            log, ndone = eng.trk_fetch_log()
            lock, losses = eng.rx_lock_status()
            hist.append(dict(wp=eng.ring_wrpos(1), status=eng.rx_status(), I=II[:, :, 0].copy(), Q=QQ[:, :, 0].copy(), log=log,
                             ndone=ndone, lock=lock, losses=losses, II=II, QQ=QQ))
        return hist
    finally:
        eng.close()


@pytest.fixture(scope="module")
def sig(gc, synth):
    return ls.signal(gc, synth)


@pytest.fixture(scope="module")
def runs(gc, sig):
    return dict(on=_run(gc, sig, True), off=_run(gc, sig, False))


@pytest.fixture(scope="module")
def verdicts(runs):
    """The restated detector over each step's fetched outputs, each channel at its own bit length, the state carried: per
    step and channel the state, the window means and whether the step declared the channel lost.  Asserts the device's
    states on the way (exact)."""
    st = [lr.zero_state() for _ in range(NCH)]
    out = []
    for k, h in enumerate(runs["on"]):
        words, mus = [], []
        for i in range(NCH):
            nd = int(h["ndone"][i])
            cnt0 = int(h["status"][i]["cnt"]) - nd
            ev = []
            lr.run(st[i], ls.PRM[i], ls.RATES[i], h["I"][i], h["Q"][i], h["log"]["flagsync"][i], h["log"]["navbit"][i], nd, cnt0,
                   events=ev)
            assert lr.same(st[i], h["lock"][i]) == [], (k, ls.PRNS[i], st[i], lr.from_struct(h["lock"][i]))
            words.append(int(any(e[0] == "lost" for e in ev)))
            mus.append([e[2] for e in ev if e[0] == "mu"])
        out.append(dict(words=words, mus=mus, st=[dict(s) for s in st]))
    return out


def _hand_overs(hist, i):
    """[(step, hand-over sample, cnt of the row in which flagsync rose or None)] of channel i: a run starts in the step
    whose first row has cnt 0."""
    out = []
    for k, h in enumerate(hist):
        nd = int(h["ndone"][i])
        if nd == 0:
            continue
        cnt0 = int(h["status"][i]["cnt"]) - nd
        if cnt0 == 0:
            out.append([k, int(h["log"]["buffloc"][i][0]), None])
        fs = h["log"]["flagsync"][i][:nd]
        if out[-1][2] is None and fs.any():
            out[-1][2] = cnt0 + int(np.argmax(fs != 0))
    return [tuple(x) for x in out]


def test_lock_status_equals_restatement_after_every_step(runs, verdicts):
    assert len(verdicts) == ls.NCHUNK and [h["wp"] for h in runs["on"]] == ls.step_wrpos()
    # the monitor saw windows at both bit lengths in the same launches: 32 bit ends per 64-row chunk beside 3 or 4
    for k in range(19, 25):
        assert all(len(verdicts[k]["mus"][i]) >= 1 for i in range(NCH)), k
    last = verdicts[-1]["st"]
    assert last[2]["windows"] >= 20 and last[2]["mu_last"] > 16.0 and last[2]["lost"] == 0
    assert last[1]["windows"] >= 15 and last[1]["mu_last"] > ls.MU_LOCKED_MIN and last[1]["lost"] == 0
    assert (last[0]["lost"], last[0]["reason"]) == (1, 2) and last[0]["windows"] >= 40


def test_status_history_follows_the_verdicts_and_the_schedule_rule(gc, runs, verdicts):
    for i, p in enumerate(ls.PRNS):
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
            word = verdicts[k]["words"][i]


def test_scenario_outcomes_against_the_oracle(gc, orc, sig, runs, verdicts):
    """What the device decides, and -- within one step -- when, against the free-running oracle."""
    on = runs["on"]
    T, S = gc.CH_TRACK, gc.CH_SEARCH
    states = lambda i: [h["status"][i]["state"] for h in on]
    lost_steps = lambda i: [k for k, v in enumerate(verdicts) if v["words"][i]]
    olost = lambda h: [e[1] for e in h["events"] if e[0] == "lost"]
    O = [ls.oracle_schedule(gc, orc, sig, i) for i in (0, 1)]
    limit = (ls.NBAD + 1) * ls.KBITS * 2 * 1e-3

    # PRN 120: the right edge as its own hand-over predicts, no loss while on, the power rule after T_OFF
    ho = _hand_overs(on, 0)
    assert len(ho) == 1 and ho[0][0] == 0
    row, synci, right, found = ls.predict(0, ho[0][1])
    assert right and ho[0][2] == row and found is not None
    kl = lost_steps(0)
    print("PRN 120 lost in step: device %s, oracle %s; PRN 133: device %s, oracle %s" % (kl, olost(O[0]), lost_steps(1), olost(O[1])))
    assert len(kl) == 1 and len(olost(O[0])) == 1 and abs(kl[0] - olost(O[0])[0]) <= 1
    st = verdicts[kl[0]]["st"][0]
    assert (st["lost"], st["reason"]) == (1, 2)
    h = on[kl[0]]
    t_lost = float(h["log"]["buffloc"][0][st["lost_cnt"] - (int(h["status"][0]["cnt"]) - int(h["ndone"][0]))]) / ls.F_SF
    assert ls.T_OFF < t_lost <= ls.T_OFF + limit, t_lost
    assert states(0) == [T] * (kl[0] + 1) + [S] * (ls.NCHUNK - kl[0] - 1) and on[-1]["status"][0]["acq"]["flagacq"] == 0
    # every window that ended before T_OFF kept the quarter of the range from mu_min that the oracle's kept
    before_off = [m for k in range(kl[0]) for m in verdicts[k]["mus"][0] if on[k]["wp"] / ls.F_SF <= ls.T_OFF]
    assert len(before_off) >= 38 and min(before_off) - ls.MU_MIN >= 0.25

    # PRN 133: the wrong edge, lost as noise by the power rule, searched again in the next step, then the right edge
    ho = _hand_overs(on, 1)
    oho = O[1]["handover"]
    assert len(ho) == len(oho) == 2 and ho[0][1] == oho[0]              # (the searches are exact: the same samples)
    first, second = ls.predict(1, ho[0][1]), ls.predict(1, ho[1][1])
    assert not first[2] and ho[0][2] == first[0] and second[2] and ho[1][2] == second[0]
    kl = lost_steps(1)
    assert len(kl) == 1 and olost(O[1]) == [9] and abs(kl[0] - 9) <= 1
    st = verdicts[kl[0]]["st"][1]
    assert (st["lost"], st["reason"], st["windows"]) == (1, 2, ls.NBAD)
    assert ho[1][0] == kl[0] + 1 and (kl[0] != 9 or ho[1][1] == oho[1]) and states(1) == [T] * ls.NCHUNK and on[-1]["losses"][1] == 1
    wrong_mus = [m for k in range(kl[0] + 1) for m in verdicts[k]["mus"][1]]
    right_mus = [m for k in range(kl[0] + 1, ls.NCHUNK) for m in verdicts[k]["mus"][1]]
    assert max(wrong_mus) <= ls.MU_MIN - 0.25 and len(right_mus) >= 20 and min(right_mus) - ls.MU_MIN >= 0.25

    # PRN 12: never lost, at its own thresholds
    assert states(2) == [T] * ls.NCHUNK and lost_steps(2) == [] and on[-1]["losses"][2] == 0


def test_frame_from_the_steps_rows(gc, engine, runs):
    """The rows of each step to gnsscorr_sbasframe_replay with the step's cnt0: PRN 120's frame at the cnt its hand-over
    predicts, the state equal to the plain replay on the same rows; PRN 133's second run finds none."""
    on = runs["on"]
    for i, run in ((0, 0), (1, 1)):
        ho = _hand_overs(on, i)[run]
        found = ls.predict(i, ho[1])[3]
        st = gc.SbasFrameState()
        sym, cnts, locs = [], [], []
        for k in range(ho[0], ls.NCHUNK):
            h = on[k]
            nd = int(h["ndone"][i])
            if nd == 0:
                break
            cnt0 = int(h["status"][i]["cnt"]) - nd
            rows = h["log"][i][:nd]
            engine.sbasframe_replay(st, rows, cnt0)
            j = np.flatnonzero(rows["navbit"])
            sym += list(rows["navbit"][j])
            cnts += list(cnt0 + j)
            locs += list(rows["buffloc"][j])
        _same(st, sic.replayed(sym, cnts, locs))
        print("PRN %d: firstsfcnt predicted %s, found %d (flagdec %d, polarity %d)" % (ls.PRNS[i], found, st.firstsfcnt, st.flagdec, st.polarity))
        if i == 0:
            assert found == 2 * (ls.LEAD + 1511) + 1 - ls.code_period(0, ho[1])
            assert (st.flagdec, st.firstsfcnt, st.firstsftow, st.week) == (1, found, ls.TOW, ls.WEEK)
            assert st.firstsf == locs[cnts.index(found)] and (st.id, st.tow) == (2, ls.TOW + 1)     # message 1, 1000 periods on
            assert bytes(st.msg) == bytes(np.packbits(np.array(sic.messages()[1] + [0] * 6, np.uint8)))
        else:
            assert found is None and st.flagtow == 0 and _fields(st) == fr.SbasReplay().fields()


def test_control_engine_without_the_monitor(gc, runs, verdicts):
    """The monitor off: every channel tracks to the end; and the monitor disturbs nothing: up to and including the step
    of its first loss every channel's sums, log rows and status are bit-identical in the two engines."""
    on, off = runs["on"], runs["off"]
    for i in range(NCH):
        assert [h["status"][i]["state"] for h in off] == [gc.CH_TRACK] * ls.NCHUNK, i
        lost = [k for k, v in enumerate(verdicts) if v["words"][i]]
        upto = lost[0] if lost else ls.NCHUNK - 1
        for k in range(upto + 1):
            a, b = on[k], off[k]
            assert a["ndone"][i] == b["ndone"][i] > 0, (i, k)
            assert a["log"][i].tobytes() == b["log"][i].tobytes(), (i, k)
            assert a["II"][i].tobytes() == b["II"][i].tobytes() and a["QQ"][i].tobytes() == b["QQ"][i].tobytes(), (i, k)
            assert a["status"][i] == b["status"][i], (i, k)
    assert all(not np.any(h["losses"]) for h in off)
    assert all(h["lock"].tobytes() == bytes(h["lock"].nbytes) for h in off)
