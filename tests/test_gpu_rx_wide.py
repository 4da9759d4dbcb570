"""The schedule's three stages together on the wide receiver of tests/rx_wide_cases.py (-m gpu): eleven channels on two
rings, the lock monitor, bit synchronisation by symbol energy and the correlation monitor on with ragged on-sets, so that
gc_rx_*_launch builds lists that are longer than one workgroup, sparse, and hold 0 rows beside 250 -- the regime of
gc_rows_of_run (csrc/gnsscorr_stage.h) that no other test enters.  tests/test_rx_wide_host.py shows on the oracle alone
that the scenario decides what is claimed here.

Engines, each run once (module fixtures):
  A  all three stages on            B  no stage (control)           C  bit synchronisation only, the same on-set
  D  A's configuration on an engine whose device buffers are poisoned with 0xA5, nothing fetched between the steps
  E  the 33-tap run (corrn 16: row_stride 33, 16 pairs), all three stages on
  F, G  lock and correlation monitors only on the recording in which Y's signal stays: F stepped at 0.1 s / 100 periods
     behind the first step, G at 0.25 s / 300

Bars, all exact: the stage states behind every step equal the restatements (tests/{lock,bsync,cfm}_restate.py) over
that step's own fetched rows, every double as bytes; losses, applied counts and the rx_status history follow the restated
verdicts through lock_cases.schedule_step; engines that differ in a stage fetch the same bytes wherever that stage may
not show."""
import numpy as np
import pytest

import bsync_restate as br
import cfm_restate as cr
import lock_restate as lr
import rx_wide_cases as wc

pytestmark = pytest.mark.gpu
T, S, I = wc.CH_TRACK, wc.CH_SEARCH, wc.CH_IDLE
LETTER = {T: "T", S: "S", I: "I"}
TIMERS = dict(lock="rx_lock", bsync="rx_bsync", cfm="rx_cfm")
RESTATE = dict(lock=lr, bsync=br, cfm=cr)
ZERO = dict(lock=lr.zero_state, bsync=br.zero_state, cfm=cr.zero_state)


def _plan(nstep):
    """[(write position of ring 1, of ring 2, max_periods)] of the scenario's steps."""
    return [(w1, w2, wc.MAX_PERIODS) for w1, w2 in wc.wrpos(nstep)]


def _cadence_plan(fast):
    """2.75 s of both rings: the first push and step as in the scenario, then 0.1 s / 100 periods (fast) or 0.25 s / 300
    per step, and one step without a push, which tracks whatever whole period a step's limit may have left behind."""
    c1, c2 = wc.CHUNK[1], wc.CHUNK[2]
    if fast:
        d1, d2 = int(0.1 * wc.RINGS[1]["f_sf"]), int(0.1 * wc.RINGS[2]["f_sf"])
        plan = [(c1, c2, wc.MAX_PERIODS)] + [(c1 + n * d1, c2 + n * d2, 100) for n in range(1, 26)]
    else:
        plan = [(c1 * n, c2 * n, wc.MAX_PERIODS) for n in range(1, 12)]
    assert plan[-1][:2] == (11 * c1, 11 * c2)
    return plan + [plan[-1]]


def _set(eng, kind, i, n, p):
    getattr(eng, "rx_%s_set" % kind)(p, ch0=i, nch=n)


def _run(gc, sigs, stages, taps=wc.TAPS, plan=None, cfm_sets=None, lock_of=None, commands=None, poison=None, fetch=True):
    """One engine through the pushes and steps of `plan` with the stages `stages` on as rx_wide_cases.initial_prm says
    and the host's commands between the steps.  Returns dict(hist=[per step: wp, status, II, QQ, ns, log, ndone, lock,
    losses, bsync, applied, cfm, loop, sync, on], final=the three status calls behind the last step, launches={stage:
    launches timed}, taps, stages, cfm_sets, commands)."""
    plan = _plan(wc.NSTEP) if plan is None else plan
    prm = wc.initial_prm(stages, cfm_sets, lock_of)
    eng = gc.Engine(0)
    try:
        if poison is not None:
            eng.debug_poison(poison)
        eng.timing(True)
        for r in (1, 2):
            eng.ring_create(r, 2, 2 * wc.CHUNK[r])
        eng.set_channels(wc.channels(gc, taps))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(wc.NCH)])
        eng.rx_start(wc.RETRY_MS)
        for i in range(wc.NCH):
            for kind in ("lock", "bsync"):
                if prm[kind][i] is not None:
                    _set(eng, kind, i, 1, prm[kind][i])
        if "cfm" in stages:
            for ch0, n, p in (wc.CFM_SETS if cfm_sets is None else cfm_sets):
                _set(eng, "cfm", ch0, n, p)
        hist, pos = [], {1: 0, 2: 0}
        for k, (w1, w2, maxp) in enumerate(plan):
            for kind, i, val in wc.apply_commands(prm, k, stages, commands):
                if kind == "rx_set":
                    eng.rx_set(i, val)
                else:
                    _set(eng, kind, i, 1, val)
            for r, w in ((1, w1), (2, w2)):
                if w > pos[r]:
                    eng.ring_push_raw(r, sigs[r][pos[r]:w], w - pos[r])
                    pos[r] = w
            eng.rx_step(maxp)
            if not fetch:
                continue
            II, QQ, ns = eng.trk_fetch()
            log, ndone = eng.trk_fetch_log()
            lock, losses = eng.rx_lock_status()
            bsync, applied = eng.rx_bsync_status()
            loops = eng.loop_get()
            hist.append(dict(wp=(eng.ring_wrpos(1), eng.ring_wrpos(2)), status=eng.rx_status(), II=II, QQ=QQ, ns=ns, log=log,
                             ndone=ndone, lock=lock, losses=losses, bsync=bsync, applied=applied, cfm=eng.rx_cfm_status(),
                             loop=[bytes(l) for l in loops], sync=[(l.flagsync, l.synci) for l in loops],
                             on={s: [p is not None for p in prm[s]] for s in wc.ALL_STAGES}))
            assert hist[-1]["wp"] == (w1, w2)
        final = dict(lock=eng.rx_lock_status(), bsync=eng.rx_bsync_status(), cfm=eng.rx_cfm_status())
        return dict(hist=hist, final=final, launches={s: eng.timing_read(TIMERS[s])[1] for s in wc.ALL_STAGES}, taps=taps,
                    stages=stages, cfm_sets=cfm_sets, lock_of=lock_of, commands=commands)
    finally:
        eng.close()


def _zero(rec):
    return rec.tobytes() == bytes(rec.nbytes)


def _restated(run):
    """The three restatements over each step's own fetched rows, the states carried, cnt0 = cnt - ndone; a set between
    the steps zeroes the named channel's state.  Asserts the device's states on the way, every channel and step (a
    channel whose stage is off or that has never tracked: zero bytes as well).  Returns per step dict(lock, bsync, cfm =
    state copies per channel, words = the lock monitor's verdicts, decided = channels the detector decided in the
    step, preset = those of them whose flagsync was still 0)."""
    prm = wc.initial_prm(run["stages"], run["cfm_sets"], run["lock_of"])
    corrn = run["taps"]["corrn"]
    st = {s: [ZERO[s]() for _ in range(wc.NCH)] for s in wc.ALL_STAGES}
    tracked = [False] * wc.NCH
    out = []
    for k, h in enumerate(run["hist"]):
        for kind, i, val in wc.apply_commands(prm, k, run["stages"], run["commands"]):
            if kind != "rx_set":
                st[kind][i] = ZERO[kind]()
        words, decided, preset = [0] * wc.NCH, [], []
        for i in range(wc.NCH):
            nd = int(h["ndone"][i])
            cnt0 = int(h["status"][i]["cnt"]) - nd
            tracked[i] = tracked[i] or nd > 0
            assert nd == 0 or h["status"][i]["state"] == T, (k, i)
            II, QQ, fs, nb = h["II"][i], h["QQ"][i], h["log"]["flagsync"][i], h["log"]["navbit"][i]
            if nd and prm["bsync"][i] is not None:
                was = st["bsync"][i]["done"]
                br.run(st["bsync"][i], prm["bsync"][i], wc.RATES[i], II[:, 0], QQ[:, 0], fs, nd, cnt0)
                if st["bsync"][i]["done"] == 1 and was == 0:
                    decided.append(i)
                    if fs[nd - 1] == 0:
                        preset.append(i)
            if nd and prm["lock"][i] is not None:
                ev = []
                lr.run(st["lock"][i], prm["lock"][i], wc.RATES[i], II[:, 0], QQ[:, 0], fs, nb, nd, cnt0, events=ev)
                words[i] = int(any(e[0] == "lost" for e in ev))
            if nd and prm["cfm"][i] is not None:
                cr.run(st["cfm"][i], cr.prm(**prm["cfm"][i]), wc.RATES[i], corrn, II, QQ, fs, nb, nd, cnt0)
            for s in wc.ALL_STAGES:
                bad = RESTATE[s].same(st[s][i], h[s][i])
                assert bad == [], (s, k, i, bad[:4])
                if prm[s][i] is None or not tracked[i] or h["status"][i]["state"] == I:
                    assert _zero(h[s][i]), (s, k, i)
        out.append(dict(lock=[dict(x) for x in st["lock"]], bsync=[br.copy_state(x) for x in st["bsync"]],
                        cfm=[cr.copy_state(x) for x in st["cfm"]], words=words, decided=decided, preset=preset))
    return out


def _lists(h):
    """Per stage the channel list of the step's launch, from rx_status and the on-sets."""
    states = [s["state"] for s in h["status"]]
    return {s: [i for i in range(wc.NCH) if h["on"][s][i] and states[i] == T] for s in wc.ALL_STAGES}


@pytest.fixture(scope="module")
def sigs(gc, synth):
    return {r: wc.signal(gc, synth, r) for r in (1, 2)}


@pytest.fixture(scope="module")
def run_a(gc, sigs):
    return _run(gc, sigs, wc.ALL_STAGES)


@pytest.fixture(scope="module")
def restated_a(run_a):
    return _restated(run_a)


@pytest.fixture(scope="module")
def run_b(gc, sigs):
    return _run(gc, sigs, ())


@pytest.fixture(scope="module")
def run_c(gc, sigs):
    return _run(gc, sigs, ("bsync",))


@pytest.fixture(scope="module")
def run_e(gc, sigs):
    return _run(gc, sigs, wc.ALL_STAGES, taps=wc.TAPS33, plan=_plan(wc.NSTEP33), cfm_sets=wc.CFM_SETS33)


@pytest.fixture(scope="module")
def restated_e(run_e):
    return _restated(run_e)


def _check_schedule(run, restated, nstep):
    """Bar 2: losses and applied per channel index, and the rx_status history by lock_cases.schedule_step applied to the
    restated verdicts and the host's commands."""
    wps = [h["wp"] for h in run["hist"]]
    for i in range(wc.NCH):
        ring = wc.RING_OF[i]
        ch = dict(state=S, next_try=wc.first_try(ring), attempts=0, losses=0)
        word, applied = 0, 0
        for k, h in enumerate(run["hist"]):
            s = h["status"][i]
            for kind, j, val in (wc.COMMANDS if run["commands"] is None else run["commands"]).get(k, []):
                if kind == "rx_set" and j == i:
                    ch["state"] = val
                    if val == S:
                        ch["next_try"] = wps[k - 1][ring - 1]

            def search(wp):
                assert s["acq_wrpos"] == wp, (i, k, s)                  # the device searched in this very step
                return bool(s["acq"]["flagacq"])

            before = dict(ch)
            searched = wc.schedule_step(ch, wps[k][ring - 1], word, search, ring)
            where = (i, k, s, ch)
            assert (s["state"], s["attempts"], int(h["losses"][i])) == (ch["state"], ch["attempts"], ch["losses"]), where
            if ch["state"] != T:
                assert h["ndone"][i] == 0, where
            if ch["state"] == S:
                assert s["next_try"] == ch["next_try"], where
            if word and before["state"] == T:
                # lost in step k - 1: searched in this very step, at this step's write position of the channel's own ring
                assert searched and s["acq_wrpos"] == wps[k][ring - 1] and ch["losses"] == before["losses"] + 1, where
            if searched and ch["state"] == T:
                assert int(s["cnt"]) == int(h["ndone"][i]) > 0, where  # cnt restarted
            word = restated[k]["words"][i]
            applied += int(i in restated[k]["preset"])
            assert int(h["applied"][i]) == applied, where
        got = "".join(LETTER[h["status"][i]["state"]] for h in run["hist"])
        assert got == wc.EXPECT_STATES[i][:nstep], (i, got)
        lost = [(k, restated[k]["lock"][i]["reason"]) for k in range(nstep) if restated[k]["words"][i]]
        assert lost == [e for e in wc.EXPECT_LOSSES.get(i, []) if e[0] < nstep], (i, lost)


def test_states_equal_the_restatements_after_every_step(run_a, restated_a):
    """Bar 1 on engine A (asserted step by step inside _restated) and what the final states hold."""
    fin = restated_a[-1]
    for s in wc.ALL_STAGES:
        rec = run_a["final"][s][0] if s != "cfm" else run_a["final"][s]
        for i in range(wc.NCH):
            assert RESTATE[s].same(fin[s][i], rec[i]) == [], (s, i)
    for i in wc.PRESENT:
        assert fin["bsync"][i]["done"] == 1, i
        if i != wc.Y:
            assert fin["lock"][i]["windows"] >= 2 and fin["lock"][i]["lost"] == 0, i
        if i != wc.CFM_GAP:
            assert fin["cfm"][i]["windows"] >= 3, (i, fin["cfm"][i]["windows"])
    alarms = [fin["cfm"][i]["alarms"] for i in wc.PRESENT if i != wc.CFM_GAP]
    assert any(a > 0 for a in alarms) and any(a == 0 for a in alarms)
    for i in wc.ABSENT + [wc.CFM_GAP]:
        assert _zero(run_a["final"]["cfm"][i]), i


def test_the_launches_were_long_sparse_and_ragged(run_a, restated_a):
    """Bar 7: the conditions that make this module mean something, from rx_status and the on-sets."""
    hist = run_a["hist"]
    lists = [_lists(h) for h in hist]
    nine = [k for k, l in enumerate(lists) if len(l["lock"]) >= 9 and len(l["bsync"]) >= 9]
    assert nine and any(k in wc.R2_SKIP for k in nine), nine
    assert max(len(l["cfm"]) for l in lists) >= 5
    for k, l in enumerate(lists):
        for s in wc.ALL_STAGES:
            assert l[s] and l[s] != list(range(len(l[s]))), (k, s)      # no list is the identity
        assert l["cfm"] != l["lock"] and l["cfm"] != l["bsync"], k
    for k in wc.R2_SKIP:
        nd = [int(x) for x in hist[k]["ndone"]]
        for s in wc.ALL_STAGES:
            assert wc.ragged(lists[k][s], nd), (k, s, lists[k][s], nd)
    reasons = [restated_a[k]["lock"][i]["reason"] for k in range(wc.NSTEP) for i in range(wc.NCH) if restated_a[k]["words"][i]]
    assert 1 in reasons and 2 in reasons
    # X's verdict sat at a list position that is another channel's index
    assert lists[2]["lock"].index(wc.X) != wc.X and restated_a[2]["words"][wc.X] == 1
    # one launch of each stage per step with a non-empty list
    for s in wc.ALL_STAGES:
        assert run_a["launches"][s] == sum(1 for l in lists if l[s]) == wc.NSTEP, s


def test_losses_applied_and_status_history_follow_the_verdicts(run_a, restated_a):
    _check_schedule(run_a, restated_a, wc.NSTEP)
    hist = run_a["hist"]
    # the parked channel: IDLE with frozen loop state, then acquired a third time
    x = [h["status"][wc.X] for h in hist]
    assert [s["attempts"] for s in x] == [1, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3, 3]
    assert hist[4]["loop"][wc.X] == hist[5]["loop"][wc.X] == hist[3]["loop"][wc.X]
    assert [int(h["losses"][wc.X]) for h in hist] == [0, 0, 0] + [1] * 9
    assert [int(h["losses"][wc.Y]) for h in hist] == [0] * 8 + [1] * 4
    assert all(int(h["losses"][i]) == 0 for h in hist for i in range(wc.NCH) if i not in (wc.X, wc.Y))
    # Y's search in vain pauses on ring 1's sample clock
    assert x[6]["acq_wrpos"] == hist[6]["wp"][0]
    y8 = hist[8]["status"][wc.Y]
    assert (y8["acq_wrpos"], y8["acq"]["flagacq"], y8["next_try"]) == (hist[8]["wp"][0], 0, hist[8]["wp"][0] + wc.retry_samples(1))


def test_presets_reach_the_loop_state_and_the_next_rows(run_a, restated_a):
    """Bar 3, for every decided channel of both rings."""
    hist = run_a["hist"]
    for i in wc.PRESENT:
        kd = [k for k in range(wc.NSTEP) if i in restated_a[k]["decided"]]
        assert len(kd) == 1 and i in restated_a[kd[0]]["preset"], (i, kd)
        kd = kd[0]
        st = restated_a[kd]["bsync"][i]
        truth = wc.true_synci(i, hist[kd]["status"][i]["acq"]["buffloc"])
        assert (st["done"], st["synci"]) == (1, truth), (i, st["synci"], truth)
        first = max(k for k in range(kd + 1) if hist[k]["status"][i]["attempts"] != (hist[k - 1]["status"][i]["attempts"] if k else 0))
        for k in range(first, wc.NSTEP):
            h = hist[k]
            if h["status"][i]["state"] != T:
                break
            nd = int(h["ndone"][i])
            assert h["sync"][i] == ((1, truth) if k >= kd else (0, 0)), (i, k, h["sync"][i])
            assert np.all(h["log"]["flagsync"][i][:nd] == (1 if k > kd else 0)), (i, k)
        assert kd == 9 if i == wc.X else kd <= 3, (i, kd)               # (all but X: before the first step that skips ring 2)


def _same_fetch(a, b, i, where, preset=None):
    """Channel i's fetches of one step on two engines; preset: engine a's loop state holds a preset of this step that
    engine b's lacks, (LoopState, flagsync, synci): b's bytes with those two fields set are a's."""
    nd = int(a["ndone"][i])
    assert nd == int(b["ndone"][i]) and a["status"][i] == b["status"][i], where
    if preset is None:
        assert a["loop"][i] == b["loop"][i], where
    else:
        l = preset[0].from_buffer_copy(b["loop"][i])
        assert (l.flagsync, l.synci) == (0, 0) and a["loop"][i] != b["loop"][i], where
        l.flagsync, l.synci = preset[1:]
        assert bytes(l) == a["loop"][i], where
    assert a["log"][i][:nd].tobytes() == b["log"][i][:nd].tobytes(), where
    for f in ("II", "QQ", "ns"):
        assert a[f][i][:nd].tobytes() == b[f][i][:nd].tobytes(), where + (f,)


def test_engines_that_differ_in_a_stage(gc, run_a, restated_a, run_b, run_c):
    """Bar 4.  C (bit synchronisation only) against A: every channel until the step whose verdict loses it in A or in
    which it is parked.  B (no stage) against A: every channel up to and including its deciding step, behind which A's
    loop state differs by the preset and by nothing else."""
    first_loss = {i: min([k for k in range(wc.NSTEP) if restated_a[k]["words"][i]] + [wc.NSTEP]) for i in range(wc.NCH)}
    decided = {i: min([k for k in range(wc.NSTEP) if i in restated_a[k]["decided"]] + [wc.NSTEP]) for i in range(wc.NCH)}
    compared = 0
    for k in range(wc.NSTEP):
        a, b, c = run_a["hist"][k], run_b["hist"][k], run_c["hist"][k]
        assert _zero(b["lock"]) and _zero(b["bsync"]) and _zero(b["cfm"]) and not np.any(b["applied"]) and not np.any(b["losses"])
        assert _zero(c["lock"]) and _zero(c["cfm"]) and not np.any(c["losses"])
        assert c["bsync"].tobytes() == a["bsync"].tobytes() or k > first_loss[wc.X], k
        for i in range(wc.NCH):
            if k <= first_loss[i] and not (i == wc.X and k >= wc.PARKED_STEPS[0]):
                _same_fetch(a, c, i, ("C", k, i))
                compared += 1
            if k <= min(decided[i], first_loss[i]):
                st = restated_a[k]["bsync"][i]
                _same_fetch(a, b, i, ("B", k, i), preset=(gc.LoopState, 1, st["synci"]) if k == decided[i] else None)
    assert compared >= 9 * wc.NSTEP
    # behind its deciding step a channel does differ: the control has not synchronised
    assert run_b["hist"][5]["sync"][0] == (0, 0) and run_a["hist"][5]["sync"][0][0] == 1
    assert run_b["launches"] == dict(lock=0, bsync=0, cfm=0)
    assert run_c["launches"] == dict(lock=0, bsync=wc.NSTEP, cfm=0)


def test_poisoned_engine_without_fetches_ends_in_the_same_states(gc, sigs, run_a):
    """Bar 5."""
    d = _run(gc, sigs, wc.ALL_STAGES, poison=0xA5, fetch=False)
    for s in wc.ALL_STAGES:
        got, want = d["final"][s], run_a["final"][s]
        if s == "cfm":
            assert got.tobytes() == want.tobytes()
        else:
            assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]), s
    assert d["launches"] == run_a["launches"]


def test_33_taps_states_schedule_and_windows(run_e, restated_e):
    """Bars 1 and 2 on engine E: row_stride 33, every lane 0 .. 32 of the correlation monitor owns a tap."""
    _check_schedule(run_e, restated_e, wc.NSTEP33)
    prm = wc.initial_prm(cfm_sets=wc.CFM_SETS33)
    fin = restated_e[-1]
    on = [i for i in wc.PRESENT if prm["cfm"][i] is not None]
    assert len(on) >= 5 and any(prm["cfm"][i]["npair"] == 16 for i in on)
    for i in on:
        st = fin["cfm"][i]
        assert st["windows"] >= 1 and st["cfP"][32] > 0.0 and np.all(st["cfP"][:33] > 0.0), (i, st["windows"])
    k = [k for k in wc.R2_SKIP if k < wc.NSTEP33][0]
    lists = _lists(run_e["hist"][k])
    for s in wc.ALL_STAGES:
        assert wc.ragged(lists[s], [int(x) for x in run_e["hist"][k]["ndone"]]), s
    assert all(fin["bsync"][i]["done"] == 1 for i in wc.PRESENT if i != wc.X)
    assert run_e["launches"] == dict(lock=wc.NSTEP33, bsync=wc.NSTEP33, cfm=wc.NSTEP33)


def test_states_are_the_same_from_cut_to_cut_through_the_schedule(gc, synth, sigs):
    """Bar 6: lock and correlation monitors only, thresholds nothing fails, Y's signal left on, so that no channel is
    lost and every L1 C/A channel synchronises by the reference's rule behind cnt 2000.  Steps of 100 rows (one chunk of
    64 and one of 36) end in the bytes that steps of 250 rows end in."""
    on = {1: wc.signal(gc, synth, 1, keep_on=True), 2: sigs[2]}
    kw = dict(lock_of=lambda i: wc.LOCK_NEVER, commands={})
    f = _run(gc, on, ("lock", "cfm"), plan=_cadence_plan(True), **kw)
    g = _run(gc, on, ("lock", "cfm"), plan=_cadence_plan(False), **kw)
    rf = _restated(f)
    for i in wc.PRESENT:                                                # (a step of 0.1 s holds 100 periods but for the odd 99 or 101)
        assert sum(int(h["ndone"][i]) == 100 for h in f["hist"][1:26]) >= 20, i
    assert f["final"]["lock"][0].tobytes() == g["final"]["lock"][0].tobytes()
    assert f["final"]["cfm"].tobytes() == g["final"]["cfm"].tobytes()
    assert not np.any(f["final"]["lock"][1]) and not np.any(g["final"]["lock"][1])
    assert [s["cnt"] for s in f["hist"][-1]["status"]] == [s["cnt"] for s in g["hist"][-1]["status"]]
    assert all(s["state"] == T for i, s in enumerate(g["hist"][-1]["status"]) if i in wc.PRESENT)
    # the states hold windows, not only zeros: every L1 C/A channel synchronised and closed some
    fin = rf[-1]
    for i in wc.PRESENT:
        w = (fin["lock"][i]["windows"], fin["cfm"][i]["windows"])
        print("channel %d: lock windows %d, cfm windows %d" % ((i,) + w))
        if wc.RATES[i] == 20:
            assert w[0] >= 2 and (w[1] >= 1 or i == wc.CFM_GAP), (i, w)
