"""The wide receiver of tests/rx_wide_cases.py on the CPU oracle and the three restatements alone (no GPU): every present
channel is searched by orc_sdracquisition when the schedule rule makes a search due and tracked by orc_sdrthread_step,
the restated lock monitor, bit-synchronisation detector and correlation monitor run over the oracle's rows, and the
detector's decision is poked into the oracle at the step boundary, as the schedule does.

Everything asserted here is a condition the scenario has to meet for tests/test_gpu_rx_wide.py to mean what it says,
not a measurement: were one to fail, the scenario's parameters change, not the condition."""
import numpy as np
import pytest

import bsync_restate as br
import cfm_restate as cr
import lock_restate as lr
import rx_wide_cases as wc

T, S, I = wc.CH_TRACK, wc.CH_SEARCH, wc.CH_IDLE
LETTER = {T: "T", S: "S", I: "I"}


@pytest.fixture(scope="module")
def sigs(gc, synth):
    return {r: wc.signal(gc, synth, r) for r in (1, 2)}


@pytest.fixture(scope="module")
def runs(orc, sigs):
    """{channel: oracle_channel(...)} of the main scenario, every channel tracked once."""
    return {i: wc.oracle_channel(orc, sigs[wc.RING_OF[i]], i) for i in range(wc.NCH)}


@pytest.fixture(scope="module")
def runs33(orc, sigs):
    return {i: wc.oracle_channel(orc, sigs[wc.RING_OF[i]], i, taps=wc.TAPS33, nstep=wc.NSTEP33, cfm_sets=wc.CFM_SETS33)
            for i in range(wc.NCH)}


def _tables(runs, nstep, cfm_sets=None):
    """Per step the states, row counts and parameter tables (the commands applied)."""
    prm = wc.initial_prm(cfm_sets=cfm_sets)
    out = []
    for k in range(nstep):
        wc.apply_commands(prm, k, wc.ALL_STAGES)
        out.append(dict(states=[runs[i]["steps"][k]["state"] for i in range(wc.NCH)],
                        ndone=[runs[i]["steps"][k]["ndone"] for i in range(wc.NCH)],
                        prm={s: list(v) for s, v in prm.items()}))
    return out


def test_every_present_satellite_is_acquired_at_its_first_attempt_and_no_absent_one_ever(runs):
    for i in wc.PRESENT:
        s0 = runs[i]["steps"][0]
        assert (s0["state"], s0["attempts"], s0["flagacq"]) == (T, 1, 1), (i, s0)
        # and at every later attempt while its signal is there
        for k, s in enumerate(runs[i]["steps"]):
            if s["searched"] and not (i == wc.Y and k > 6):
                assert s["flagacq"] == 1 and s["state"] == T, (i, k)
    for i in wc.ABSENT:
        steps = runs[i]["steps"]
        assert all(s["state"] == S and s["ndone"] == 0 for s in steps) and steps[-1]["attempts"] == 2, i
    # the absent PRNs are searched again in different steps: RETRY_MS later on each ring's own sample clock
    again = {i: [k for k, s in enumerate(runs[i]["steps"]) if s["searched"]] for i in wc.ABSENT}
    assert again == {4: [0, 6], 8: [0, 8]}


def test_state_history_is_the_one_the_gpu_test_expects(runs):
    """lc.schedule_step applied to the restated verdicts and the host's commands."""
    for i in range(wc.NCH):
        got = "".join(LETTER[s["state"]] for s in runs[i]["steps"])
        print("channel %2d %-12s %s  losses %s  hand-overs %s" % (i, wc.CH[i][0], got, runs[i]["lost"], runs[i]["handover"]))
        assert got == wc.EXPECT_STATES[i], i
        assert [(k, reason) for k, _, reason in runs[i]["lost"]] == wc.EXPECT_LOSSES.get(i, []), (i, runs[i]["lost"])
    for k in wc.PARKED_STEPS:
        assert runs[wc.X]["steps"][k]["state"] == I and runs[wc.X]["steps"][k]["ndone"] == 0


def test_lists_are_long_sparse_and_ragged(runs):
    tabs = _tables(runs, wc.NSTEP)
    lists = [wc.lists(t["states"], t["prm"]) for t in tabs]
    for k, l in enumerate(lists):
        print("step %2d rows %s" % (k, tabs[k]["ndone"]), {s: v for s, v in l.items()})
    # three workgroups, the last one partial: nine entries in the lock monitor's and the detector's list of one step
    nine = [k for k, l in enumerate(lists) if len(l["lock"]) >= 9 and len(l["bsync"]) >= 9]
    assert nine and any(k in wc.R2_SKIP for k in nine), nine
    assert max(len(l["cfm"]) for l in lists) >= 5
    # the lists differ from the identity in every step, the correlation monitor's from the other two in every step, the
    # lock monitor's from the detector's while X tracks without the detector
    for k, l in enumerate(lists):
        assert l["lock"] != l["bsync"] or k >= wc.PARKED_STEPS[0], k
        assert l["cfm"] != l["lock"] and l["cfm"] != l["bsync"], k
        for s in wc.ALL_STAGES:
            assert l[s] != list(range(len(l[s]))), (k, s)
    # a step that skips ring 2: its channels stay in TRACK with 0 rows beside ring 1 channels with 250
    for k in wc.R2_SKIP:
        nd = tabs[k]["ndone"]
        for i in wc.PRESENT:
            if tabs[k]["states"][i] == T:                              # (X is handed over in step 6, ten periods before its end)
                assert nd[i] == (0 if wc.RING_OF[i] == 2 else 10 if runs[i]["steps"][k]["searched"] else 250), (k, i, nd)
        for s in wc.ALL_STAGES:
            assert wc.ragged(lists[k][s], nd), (k, s, lists[k][s], nd)
    # 250 rows everywhere else behind the first step
    assert all(tabs[k]["ndone"][0] == 250 for k in range(1, wc.NSTEP))


def test_bit_sync_decides_the_true_edge_and_the_lock_monitor_loses_x_and_y(runs):
    for i in wc.PRESENT:
        r = runs[i]
        print("channel %2d decided %s applied %d" % (i, r["decided"], r["steps"][-1]["applied"]))
        assert len(r["decided"]) == 1 and r["decided"][0][1] == r["decided"][0][2], (i, r["decided"])
        assert r["steps"][-1]["bsync"]["done"] == 1 and r["steps"][-1]["applied"] == 1, i
        kd = r["decided"][0][0]
        assert r["steps"][kd]["loop"] == (1, r["decided"][0][1])
        if i != wc.X:
            assert kd <= 3, (i, kd)                                      # before the first step that skips ring 2
    x = runs[wc.X]
    # X: no detector, lost by the time limit, tracks again with a cnt that restarted; decided only in its third run
    assert x["lost"] == [(2, wc.LOCK_X0["sync_periods"] - 1, 1)] and x["decided"][0][0] >= 7
    assert [k for k, _ in x["handover"]] == [0, 3, 6]
    assert x["steps"][3]["cnt"] == x["steps"][3]["ndone"] > 0 and x["steps"][6]["cnt"] == x["steps"][6]["ndone"] > 0
    # parked with every stage state still zero
    s = x["steps"][wc.PARKED_STEPS[-1]]
    assert s["lock"] == lr.zero_state() and s["bsync"] == br.zero_state()
    assert not any(np.any(s["cfm"][f]) for f in cr.FIELDS)
    # Y: lost by the power rule within 0.3 s of the end of its signal, searched in vain in the next step
    y = runs[wc.Y]
    assert [(k, reason) for k, _, reason in y["lost"]] == [(7, 2)]
    assert y["steps"][8]["searched"] and y["steps"][8]["flagacq"] == 0 and y["steps"][-1]["attempts"] == 2
    for i in wc.PRESENT:
        if i not in (wc.X, wc.Y):
            assert runs[i]["lost"] == [] and runs[i]["steps"][-1]["lock"]["windows"] >= 2, i


def test_correlation_monitor_windows_and_alarms(runs, runs33):
    prm = wc.initial_prm()
    on = [i for i in wc.PRESENT if prm["cfm"][i] is not None]
    assert wc.CFM_GAP not in on and wc.CFM_GAP in wc.PRESENT and min(on) < wc.CFM_GAP < max(on)
    alarms = {}
    for i in on:
        st = runs[i]["steps"][-1]["cfm"]
        alarms[i] = st["alarms"]
        print("channel %2d windows %d alarms %d" % (i, st["windows"], st["alarms"]))
        assert st["windows"] >= 3, (i, st["windows"])
    assert any(a > 0 for a in alarms.values()) and any(a == 0 for a in alarms.values())
    # the loose set has no bad window while the signal is there, the tight set has some
    loose_bad = [e for i in range(0, 6) if i != wc.Y for e in runs[i]["cfm_events"] if e[5]]
    tight_bad = [e for i in range(7, 11) for e in runs[i]["cfm_events"] if e[5]]
    assert not loose_bad and tight_bad
    # 33 taps: at least one window for every channel with the monitor on, all 16 pairs on the first set
    prm33 = wc.initial_prm(cfm_sets=wc.CFM_SETS33)
    on33 = [i for i in wc.PRESENT if prm33["cfm"][i] is not None]
    assert wc.X not in on33 and len(on33) >= 5
    for i in on33:
        st = runs33[i]["steps"][-1]["cfm"]
        print("33 taps: channel %2d windows %d, ratio %s" % (i, st["windows"], st["ratio"][:16].round(2)))
        assert st["windows"] >= 1, i
    assert any(prm33["cfm"][i]["npair"] == 16 for i in on33)
    # lane 32's tap is summed: the outermost pair has values of its own
    assert all(runs33[i]["steps"][-1]["cfm"]["cfP"][32] > 0.0 for i in on33)


def test_the_33_tap_run_has_the_same_schedule_and_a_ragged_step(runs33):
    tabs = _tables(runs33, wc.NSTEP33, wc.CFM_SETS33)
    for i in range(wc.NCH):
        got = "".join(LETTER[s["state"]] for s in runs33[i]["steps"])
        assert got == wc.EXPECT_STATES[i][:wc.NSTEP33], (i, got)
    k = [k for k in wc.R2_SKIP if k < wc.NSTEP33][0]
    l = wc.lists(tabs[k]["states"], tabs[k]["prm"])
    for s in wc.ALL_STAGES:
        assert wc.ragged(l[s], tabs[k]["ndone"]), (s, l[s], tabs[k]["ndone"])
    for i in wc.PRESENT:
        if i != wc.X:
            assert len(runs33[i]["decided"]) == 1 and runs33[i]["decided"][0][1] == runs33[i]["decided"][0][2], i
