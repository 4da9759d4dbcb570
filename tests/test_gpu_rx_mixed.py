"""The receiver schedule on mixed front ends (-m gpu): the device hand-over of every channel type, the schedule on
two rings at different paces against the CPU oracle, and its edges.  Scenarios: tests/rx_mixed_cases.py;
tests/test_rx_mixed_host.py shows on the oracle alone that they decide what is claimed here.

Bars: those of tests/test_gpu_rx.py and tests/test_gpu_loop_mixed.py -- search integers and buffloc exact, peakr / cn0
to 1e-4; currnsamp, II / QQ, remainders, filter flags, flagsync and navbit of every tracked period exact; filter
outputs under _adopt to 1e-14 for L1 C/A on the 16.368 Msps IQ ring and 1e-12 for G1, SBAS, 13-tap and 20 Msps
channels; state, attempts, next_try, acq_wrpos and cnt at every step."""
import ctypes as C

import numpy as np
import pytest

import rx_cases as rc
import rx_mixed_cases as mc
from test_gpu_loop import _adopt, _check_against_oracle, _signal

pytestmark = pytest.mark.gpu
NS = 16368


# ---- hand-over of every channel type -------------------------------------------------------------------------------
def _preset_loop(e, i, acqfreq):
    """A loop state whose every running field is non-zero, up to the last element of every array."""
    ls = e.loop_state(i, acqfreq, flagsync=1, synci=3 + i, cnt=4000 + i)
    ls.navcnt, ls.swloop, ls.carrNco, ls.codeNco, ls.carrErr, ls.codeErr, ls.freqErr = 7, 1, 1.5, -0.25, 0.1, 0.2, 0.3
    ls.biti, ls.bit, ls.swsync, ls.swreset, ls.flagpol, ls.bitIP = 5, -1, 1, 1, 1, 123.0
    for j, name in enumerate(("II", "QQ", "oldI", "oldQ", "sumI", "sumQ", "oldsumI", "oldsumQ")):
        a = getattr(ls, name)
        for k in range(len(a)):
            a[k] = 10.0 * (j + 1) + k + 0.5
    for k in range(20):
        ls.bitsync[k] = k + 1
    return ls


def test_handover_of_every_channel_type(gc, orc, synth, engine):
    """One engine on two rings: L1 C/A with 13 taps and SBAS on real samples at a 4.092 MHz IF, G1 with frequency
    numbers +2 and -3 and an RTL-SDR replay channel (ppmerr 30: foffset 47.3 kHz) on int8 IQ; one channel with a
    satellite is not listed, one L1 C/A and one G1 channel find nothing.  Every running field of every loop state is
    non-zero before the search.  Device hand-over = host hand-over byte for byte (acquired: reset, crate from the
    channel -- 0.511 MHz for G1; failed and unlisted: untouched), 200 periods equal on both engines, and those
    periods and 1900 more against the oracle from the hand-over state -- the SBAS channel through its symbol
    synchronisation into filter updates every 2 periods."""
    sig = {r: mc.hand_signal(gc, synth, r) for r in (1, 2)}
    chans = [mc.hand_channel(gc, s) for s in mc.HAND]
    nch = len(chans)
    assert chans[6].foffset == mc.RTL_OFFSET and [c.crate for c in chans[4:6]] == [0.511e6] * 2 and chans[0].ntap == 13
    parked = [i for i in range(nch) if i not in mc.HAND_ACQUIRED]
    far = 10 ** 9                                                    # beyond both rings' data: a channel there plans nothing

    def prepare(e):
        for r in (1, 2):
            e.ring_create(r, mc.HAND_RINGS[r]["dtype"], sig[r].shape[0])
            e.ring_push_raw(r, sig[r], sig[r].shape[0])
        e.set_channels(chans)
        e.trk_set_state([dict(carrfreq=c.f_if + c.foffset + 900.0 + i, codefreq=c.crate + 0.25 * (i + 1), remcode=0.125 * (i + 1),
                              remcarr=0.5 + i, buffloc=(far if i in parked else 3000) + 17 * i) for i, c in enumerate(chans)])
        e.loop_set([_preset_loop(e, i, c.f_if + c.foffset + 800.0 + i) for i, c in enumerate(chans)])
        e.acq_run(mc.HAND_WRPOS, channels=mc.HAND_LISTED)

    host = gc.Engine(0)
    try:
        prepare(engine)
        prepare(host)
        before_loop = [bytes(x) for x in engine.loop_get()]
        before_trk = engine.trk_get_state()
        engine.loop_start_from_acq()
        res = host.acq_fetch()
        assert [i for i, r in enumerate(res) if r["flagacq"]] == mc.HAND_ACQUIRED, res
        for i, r in enumerate(res):
            if r["flagacq"]:
                host.loop_set([host.loop_state(i, r["acqfreq"])], ch0=i)
        host.trk_start_from_acq()
        dl, hl = engine.loop_get(), host.loop_get()
        dt, ht = engine.trk_get_state(), host.trk_get_state()
        for i, c in enumerate(chans):
            assert bytes(dl[i]) == bytes(hl[i]), (i, mc.HAND[i][0])
            assert dt[i] == ht[i], (i, dt[i], ht[i])
            if i in parked:
                assert bytes(dl[i]) == before_loop[i] and dt[i] == before_trk[i], i
            else:
                assert dl[i].acqfreq == res[i]["acqfreq"] and dl[i].cnt == 0 and dl[i].flagsync == 0 and dl[i].prn == c.prn
                assert dl[i].oldsumQ[32] == 0.0 and dl[i].bitsync[19] == 0 and dl[i].crate == c.crate
                assert dt[i] == dict(carrfreq=res[i]["acqfreq"], codefreq=c.crate, remcode=0.0, remcarr=0.0,
                                     buffloc=res[i]["buffloc"])
        # the oracle from the hand-over state
        rings = {r: orc.make_ring(sig[r], sig[r].shape[0], sig[r].shape[0]) for r in (1, 2)}
        ochs, bufflocs = [], []
        for i, s in enumerate(mc.HAND):
            o = mc.hand_oracle_channel(orc, s)
            st = dt[i]
            o.acq.acqfreq = res[i]["acqfreq"] if i not in parked else 0.0
            o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
            ochs.append(o)
            bufflocs.append(C.c_uint64(st["buffloc"]))
        oring = [rings[c.ftype] for c in chans]
        host.trk_run_loop(mc.HAND_RUNS[0])
        ndone = _check_against_oracle(orc, engine, ochs, oring, bufflocs, mc.HAND_RUNS[0], 13, tol=1e-12, stops=True)
        assert [int(x) for x in ndone] == [0 if i in parked else mc.HAND_RUNS[0] for i in range(nch)], ndone
        for a, b in zip(engine.trk_fetch() + engine.trk_fetch_log(), host.trk_fetch() + host.trk_fetch_log()):
            assert a.tobytes() == b.tobytes()
        assert [bytes(x) for x in engine.loop_get()] == [bytes(x) for x in host.loop_get()]
        assert engine.trk_get_state() == host.trk_get_state()
        ndone = _check_against_oracle(orc, engine, ochs, oring, bufflocs, mc.HAND_RUNS[1], 13, done=mc.HAND_RUNS[0],
                                      tol=1e-12, stops=True)
        assert ndone[0] == ndone[1] == mc.HAND_RUNS[1] and all(5 <= ndone[i] <= 30 for i in (4, 5, 6)), ndone
        log, _ = engine.trk_fetch_log()
        f = log[1]["flagloopfilter"]
        first2 = int(np.argmax(f == 2))
        assert ochs[1].flagsync == 1 and f[first2] == 2 and list(f[first2:first2 + 6]) == [2, 0, 2, 0, 2, 0], first2
        assert np.all(log[0]["flagloopfilter"] == 1)                # (L1 C/A: 20-period bits, not synchronised yet)
        for i in parked:
            assert bytes(engine.loop_get()[i]) == before_loop[i], i
        for i, want in ((0, 4.092e6 + 1517.0), (1, 4.092e6 - 830.0)):
            assert abs(ochs[i].carrfreq - want) < 30.0, (i, ochs[i].carrfreq)
    finally:
        host.close()


# ---- replay of one channel's schedule through the oracle -----------------------------------------------------------
def _record(eng, max_periods, rings=(1, 2)):
    II, QQ, ns = eng.trk_fetch()
    log, ndone = eng.trk_fetch_log()
    return dict(wp=tuple(eng.ring_wrpos(r) if r in rings else 0 for r in (1, 2)), status=eng.rx_status(), II=II, QQ=QQ,
                ns=ns, log=log, ndone=ndone, lapped=eng.trk_loop_lapped())


def _replay(gc, orc, o, ring, ftype, hist, i, first_try, retry, max_periods, tol, tag, state0=None):
    """Channel i of the recorded steps `hist` through the oracle channel o on its ring: sdrthread()'s state machine
    (search when due, retry after `retry` samples, then one period after the other up to max_periods a step).
    Returns (attempts, the steps in which it tracked, periods tracked in each step)."""
    L = orc.lib()
    ntap = hist[0]["II"].shape[2]
    state, next_try, attempts = state0 or (gc.CH_SEARCH, first_try, 0)
    buffloc = C.c_uint64(0)
    track_steps, periods = [], []
    for k, h in enumerate(hist):
        wp, st = h["wp"][ftype - 1], h["status"][i]
        if state == gc.CH_SEARCH and wp >= next_try and wp >= first_try:
            attempts += 1
            b, iters = rc.oracle_search(orc, o, ring, wp)
            a = st["acq"]
            where = (tag, k, a, o.acq.peakr)
            assert st["attempts"] == attempts and st["acq_wrpos"] == wp, where
            assert a["flagacq"] == o.flagacq and a["iters"] == iters and a["buffloc"] == b, where
            assert a["acqcodei"] == o.acq.acqcodei and a["freqi"] == o.acq.freqi and a["acqfreq"] == o.acq.acqfreq, where
            assert abs(a["peakr"] - o.acq.peakr) <= 1e-4 * o.acq.peakr, where
            assert abs(a["cn0"] - o.acq.cn0) <= 1e-4 * abs(o.acq.cn0), where
            if o.flagacq:
                state = gc.CH_TRACK
                buffloc.value = b
            else:
                next_try = wp + retry
        assert st["state"] == state and st["attempts"] == attempts, (tag, k, st)
        if state == gc.CH_SEARCH:
            assert st["next_try"] == next_try, (tag, k, st, next_try)
        II, QQ, ns, log, ndone = h["II"][i], h["QQ"][i], h["ns"][i], h["log"][i], int(h["ndone"][i])
        e = 0
        if state == gc.CH_TRACK:
            track_steps.append(k)
            ring.wrpos = wp
            while e < max_periods and L.orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(buffloc)):
                where = (tag, k, e)
                assert ns[e] == o.currnsamp and log[e]["currnsamp"] == o.currnsamp, where
                assert np.array_equal(II[e], np.ctypeslib.as_array(o.II)[:ntap]), where
                assert np.array_equal(QQ[e], np.ctypeslib.as_array(o.QQ)[:ntap]), where
                r = log[e]
                assert r["flagloopfilter"] == o.flagloopfilter, where
                assert r["remcode"] == o.remcode and r["remcarr"] == o.remcarr, where
                _adopt(o, r, where, tol)
                e += 1
            assert st["cnt"] == o.cnt, (tag, k)
            periods.append(e)
        assert ndone == e, (tag, k, ndone, e)
        assert np.all(ns[e:] == 0) and not np.any(II[e:]) and not np.any(QQ[e:]), (tag, k)
        assert log[e:].tobytes() == bytes(log[e:].nbytes), (tag, k)
    return attempts, track_steps, periods


# ---- the schedule on two rings ---------------------------------------------------------------------------------------
def _run_mix(gc, eng, sig, idx):
    """The scenario's pushes and steps with the channels MIX[idx]; only the rings those channels use exist."""
    specs = [mc.MIX[j] for j in idx]
    rings = sorted({s[3] for s in specs})
    for r in rings:
        eng.ring_create(r, mc.RINGS[r]["dtype"], 2 * (mc.C1 if r == 1 else mc.C2))
    eng.set_channels([mc.mix_channel(gc, s) for s in specs])
    eng.loop_set([eng.loop_state(i, 0.0) for i in range(len(specs))])
    eng.rx_start(mc.RETRY_MS)
    for s, st in zip(specs, eng.rx_status()):
        assert st["state"] == gc.CH_SEARCH and st["attempts"] == 0 and st["next_try"] == mc.first_try(s), (s[0], st)
    hist, pos = [], {1: 0, 2: 0}
    for k, want in enumerate(mc.mix_wrpos()):
        for r in rings:
            n = want[r - 1] - pos[r]
            if n:
                eng.ring_push_raw(r, sig[r][pos[r]:pos[r] + n], n)
                pos[r] += n
        eng.rx_step(mc.MAX_PERIODS)
        hist.append(_record(eng, mc.MAX_PERIODS, rings))
    return hist


ALONE = {"l1_present": 0, "r2_l1_present": 5}


@pytest.fixture(scope="module")
def mix(gc, synth):
    sig = {r: mc.mix_signal(gc, synth, r) for r in (1, 2)}
    out = {"sig": sig}
    for name, idx in [("all", list(range(len(mc.MIX))))] + [(n, [j]) for n, j in ALONE.items()]:
        eng = gc.Engine(0)
        try:
            out[name] = _run_mix(gc, eng, sig, idx)
        finally:
            eng.close()
    return out


def test_mixed_schedule_against_oracle(gc, orc, mix):
    """Nine channels on two rings whose write positions never move in step (rx_mixed_cases.MIX): every channel's
    recorded schedule replayed through the oracle on its own ring.  The first try after (intg + 1) * nsamp of the
    channel's own grid (4 periods for the intg 3 channel: searched in step 0, the others not before step 1), retries
    int(283 * 1e-3 * f_sf) samples of its own ring after the failure, ring 2's channels not due while ring 1's
    retry; searches, every tracked period and the status of every step as the oracle's."""
    sig, hist = mix["sig"], mix["all"]
    assert [h["wp"] for h in hist] == mc.mix_wrpos()
    assert all(h["lapped"] == 0 for h in hist)
    for i, spec in enumerate(mc.MIX):
        name, ctype, prn, r = spec[:4]
        ring = orc.make_ring(sig[r], sig[r].shape[0], 0)
        o = mc.mix_oracle_channel(orc, spec)
        retry = int(mc.RETRY_MS * 1e-3 * mc.RINGS[r]["f_sf"])            # the documented formula, in double
        tol = 1e-14 if (r == 1 and ctype == mc.CTYPE_L1CA) else 1e-12
        attempts, track_steps, periods = _replay(gc, orc, o, ring, r, hist, i, mc.first_try(spec), retry, mc.MAX_PERIODS,
                                                 tol, name)
        due, at = mc.MIX_DUE[name], mc.MIX_ACQUIRED_AT[name]
        assert attempts == len(due), (name, attempts)
        assert [k for k, h in enumerate(hist) if h["status"][i]["acq_wrpos"] == h["wp"][r - 1] and
                (hist[k - 1]["status"][i]["attempts"] if k else 0) < h["status"][i]["attempts"]] == due, name
        if at is None:
            assert track_steps == [], name
            continue
        assert track_steps == list(range(due[at - 1], mc.NSTEP)), (name, track_steps)
        # the channel keeps up with its ring: a chunk's periods in every step that pushed it, next to none otherwise
        per_chunk = (mc.C1 // mc.N1) if r == 1 else (mc.C2 // mc.N2)
        for k, e in zip(track_steps[1:], periods[1:]):
            pushed = r == 1 or k in mc.R2_STEPS
            assert (e >= per_chunk - 1) if pushed else (e <= 1), (name, k, e)
        want = mc.RINGS[r]["f_if"] + (0.5625e6 * prn if ctype == mc.CTYPE_G1 else 0.0) + spec[5]
        # (the search leaves the carrier within half a bin, 100 Hz at the finest grid; the loops must not walk away)
        assert abs(o.carrfreq - want) < 100.0, (name, o.carrfreq, want)


@pytest.mark.parametrize("name", list(ALONE))
def test_mixed_schedule_first_search_channel_alone(mix, name):
    """A channel acquired at its first search, in the nine-channel run and alone on a second engine that has only
    its ring, with the same pushes: tracking outputs, schedule state and the search's integers bit for bit the same in
    every step -- the steps in which other channels and the other ring were searched included.  (peakr and cn0 are
    held to 1e-4 only: with ring 2 in the engine every channel is searched by the 65536-point transform, alone on
    ring 1 by the 32768-point one, and the two round differently; measured 4e-8 relative on cn0.)"""
    i = ALONE[name]
    for k, (a, b) in enumerate(zip(mix["all"], mix[name])):
        assert a["ndone"][i] == b["ndone"][0], k
        assert a["log"][i].tobytes() == b["log"][0].tobytes(), k
        for f in ("II", "QQ", "ns"):
            assert a[f][i].tobytes() == b[f][0].tobytes(), (k, f)
        sa, sb = dict(a["status"][i]), dict(b["status"][0])
        qa, qb = dict(sa.pop("acq")), dict(sb.pop("acq"))
        for f in ("peakr", "cn0"):
            x, y = qa.pop(f), qb.pop(f)
            assert abs(x - y) <= 1e-4 * abs(y), (k, f, x, y)
        assert sa == sb and qa == qb, (k, sa, sb, qa, qb)
    assert sum(int(h["ndone"][0]) for h in mix[name]) > 400


# ---- edges -----------------------------------------------------------------------------------------------------------
PRNS, DOP, CPH = [5, 12], [1517.0, -3222.0], [311.3, 12.8]


def _two(gc, synth, engine, nper, ringlen=None, chans=None):
    sig = _signal(gc, synth, PRNS, DOP, CPH, nper)
    engine.ring_create(1, 2, ringlen or sig.shape[0])
    engine.set_channels(chans or [gc.Channel(p, dtype=2, f_if=0.0) for p in PRNS])
    engine.loop_set([engine.loop_state(i, 0.0) for i in range(2)])
    return sig


def test_backlog_longer_than_max_periods(gc, orc, synth, engine):
    """The channels are acquired on the first 12 code periods and start 11 periods back, where the search window
    began; 48 more periods arrive at once and max_periods is 10: 10 periods a step for five steps
    (ndone == max_periods), then the rest, then nothing where the data ends; every period still the oracle's."""
    sig = _two(gc, synth, engine, 60)
    n = sig.shape[0]
    engine.rx_start()
    hist = []
    for k in range(8):
        if k < 2:
            a, b = (0, 12 * NS) if k == 0 else (12 * NS, n)
            engine.ring_push_raw(1, sig[a:b], b - a)
        engine.rx_step(10)
        hist.append(_record(engine, 10, (1,)))
    for i, p in enumerate(PRNS):
        o = orc.make_chan(p, dtype=2, f_if=0.0)
        attempts, track_steps, periods = _replay(gc, orc, o, orc.make_ring(sig, n, 0), 1, hist, i, 11 * NS,
                                                 int(2000 * 1e-3 * 16.368e6), 10, 1e-14, p)
        assert attempts == 1 and track_steps == list(range(8)), (p, attempts, track_steps)
        assert periods[:5] == [10] * 5 and 0 < periods[5] < 10 and periods[6:] == [0, 0], (p, periods)
        assert 57 <= sum(periods) <= 59, (p, periods)


def test_step_after_a_batched_run_left_a_look_ahead_plan(gc, orc, synth, engine):
    """gnsscorr_trk_run plans the next batch ahead while it correlates this one; a step with due channels must retire
    that plan before the hand-over writes the tracking state (gc_quiesce): after two batched runs from hand-set
    states, rx_start and one step acquire both channels and track them from the hand-over state as the oracle does,
    not from where the batches or their look-ahead plan left them."""
    sig = _two(gc, synth, engine, 60)
    n = sig.shape[0]
    engine.ring_push_raw(1, sig, n)
    engine.trk_set_state([dict(carrfreq=1000.0 + 500 * i, codefreq=1.023e6, remcode=0.25, remcarr=0.5, buffloc=20 * NS + 999 * i)
                          for i in range(2)])
    engine.trk_run(3)
    engine.trk_run(3)
    engine.trk_fetch()
    engine.rx_start()
    hist = []
    for _ in range(2):
        engine.rx_step(30)
        hist.append(_record(engine, 30, (1,)))
    for i, p in enumerate(PRNS):
        o = orc.make_chan(p, dtype=2, f_if=0.0)
        attempts, track_steps, periods = _replay(gc, orc, o, orc.make_ring(sig, n, 0), 1, hist, i, 11 * NS,
                                                 int(2000 * 1e-3 * 16.368e6), 30, 1e-14, p)
        assert attempts == 1 and 9 <= periods[0] <= 10 and periods[1] == 0, (p, periods)


def test_restart_and_set_channels(gc, synth, engine):
    """rx_start a second time: every channel SEARCH with attempts 0 and its first try, all due at the next step, which
    acquires them again with the first step's result (same write position).  set_channels after rx_start: every rx_*
    call refuses until the next rx_start, which needs loop constants again."""
    sig = _two(gc, synth, engine, 40)
    n = sig.shape[0]
    engine.rx_start(700)
    engine.ring_push_raw(1, sig, n)
    engine.rx_step(60)
    st1 = engine.rx_status()
    assert [s["state"] for s in st1] == [gc.CH_TRACK] * 2 and [s["attempts"] for s in st1] == [1, 1]
    engine.rx_start()
    st = engine.rx_status()
    zero = dict(acqcodei=0, freqi=0, acqfreq=0.0, cn0=0.0, peakr=0.0, flagacq=0, iters=0, buffloc=0)
    for s in st:
        assert (s["state"], s["attempts"], s["next_try"], s["acq_wrpos"], s["acq"]) == (gc.CH_SEARCH, 0, 11 * NS, 0, zero), s
    engine.rx_step(60)
    st2 = engine.rx_status()
    _, ndone = engine.trk_fetch_log()
    for a, b in zip(st1, st2):
        assert b["state"] == gc.CH_TRACK and b["attempts"] == 1 and b["acq_wrpos"] == n and b["acq"] == a["acq"], (a, b)
        assert b["cnt"] == a["cnt"]                                  # the same periods again, from cnt 0
    assert np.all(ndone == [s["cnt"] for s in st2]) and np.all(ndone >= 9)
    engine.set_channels([gc.Channel(p, dtype=2, f_if=0.0) for p in PRNS])
    for call in (lambda: engine.rx_step(10), engine.rx_status, lambda: engine.rx_set(0, gc.CH_IDLE)):
        with pytest.raises(gc.GnsscorrError):
            call()
    with pytest.raises(gc.GnsscorrError):
        engine.rx_start()                                            # no loop constants yet
    engine.loop_set([engine.loop_state(i, 0.0) for i in range(2)])
    engine.rx_start()
    assert [(s["state"], s["attempts"]) for s in engine.rx_status()] == [(gc.CH_SEARCH, 0)] * 2
    engine.rx_step(60)
    assert [s["acq"] for s in engine.rx_status()] == [s["acq"] for s in st1]


def test_ring_shorter_than_one_channels_look_back(gc, synth, engine):
    """A ring of 8 code periods under a channel that looks back 11 (intg 10) beside one that looks back 4 (intg 3).
    The step refuses as a whole with the search's error, which names the ring and the look-back, and changes nothing:
    no attempt is counted, nobody is searched or tracked.  With the impossible channel parked (IDLE) the next step
    serves the other one.  """
    chans = [gc.Channel(PRNS[0], dtype=2, f_if=0.0), gc.Channel(PRNS[1], dtype=2, f_if=0.0, hband=4000, step=500, intg=3)]
    sig = _two(gc, synth, engine, 20, ringlen=8 * NS, chans=chans)
    engine.rx_start()
    for k in range(4):
        engine.ring_push_raw(1, sig[k * 5 * NS:(k + 1) * 5 * NS], 5 * NS)
        if k < 2:
            engine.rx_step(20)                                       # 5 and 10 periods: channel 1 alone is due, and found
    st = engine.rx_status()
    assert st[0]["state"] == gc.CH_SEARCH and st[0]["attempts"] == 0 and st[1]["state"] == gc.CH_TRACK
    engine.rx_set(1, gc.CH_SEARCH)
    before = engine.rx_status()
    frozen = ([bytes(x) for x in engine.loop_get()], engine.trk_get_state())
    for _ in range(2):
        with pytest.raises(gc.GnsscorrError, match="shorter than the 11 code periods"):
            engine.rx_step(20)
        assert engine.rx_status() == before
        assert ([bytes(x) for x in engine.loop_get()], engine.trk_get_state()) == frozen
    engine.rx_set(0, gc.CH_IDLE)
    engine.rx_step(20)
    st = engine.rx_status()
    assert st[0]["state"] == gc.CH_IDLE and st[0]["attempts"] == 0
    assert st[1]["state"] == gc.CH_TRACK and st[1]["attempts"] == 2 and st[1]["acq_wrpos"] == 20 * NS
    assert abs(st[1]["acq"]["acqfreq"] - DOP[1]) <= 500.0


def test_retry_pause_is_the_documented_double_formula(gc, engine):
    """retry_ms 1025 at 16.368 Msps: (double)1025 * 1e-3 * 16.368e6 is 16777199.999999998, so the documented formula
    gives a pause of 16777199 samples where exact arithmetic gives 16777200 (1025 and 2050 are the only values up to
    3000 ms at which the two differ, at either rate of these tests).  A channel on noise fails its first search."""
    retry = int(1025 * 1e-3 * 16.368e6)
    assert retry == 1025 * 16368 - 1
    rng = np.random.default_rng(8)
    n = 12 * NS
    engine.ring_create(1, 2, n)
    engine.set_channels([gc.Channel(9, dtype=2, f_if=0.0)])
    engine.loop_set([engine.loop_state(0, 0.0)])
    engine.rx_start(1025)
    engine.ring_push_raw(1, np.clip(np.rint(rng.normal(0.0, 8.0, (n, 2))), -127, 127).astype(np.int8), n)
    engine.rx_step(5)
    st = engine.rx_status()[0]
    assert st["state"] == gc.CH_SEARCH and st["attempts"] == 1 and st["acq"]["flagacq"] == 0 and st["acq"]["peakr"] < 2.0, st
    assert st["acq_wrpos"] == n and st["next_try"] == n + retry, (st, retry)


def test_research_of_a_tracking_channel_whose_satellite_has_gone(gc, orc, synth, engine):
    """PRN 5 stops after 60 code periods (synth t_off); at 80 periods its tracking channel is sent back to SEARCH.  The
    search at 100 periods fails as the oracle's does, the state stays SEARCH, loop and tracking state stay frozen
    byte for byte, the retry comes 30 ms of samples later (not at the step in between) and fails again; PRN 12's
    channel tracks through all of it exactly as the oracle, which never hears of channel 0."""
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in PRNS}
    rng = np.random.default_rng(61)
    sats = [dict(prn=p, doppler=d, codephase=c, cn0=47.0, phase=0.4 * i, bits=rng.choice([-1.0, 1.0], size=64))
            for i, (p, d, c) in enumerate(zip(PRNS, DOP, CPH))]
    sats[0]["t_off"] = 60e-3
    n = 160 * NS
    sig = synth.make_if(codes, n, f_sf=16.368e6, f_if=0.0, dtype=2, sats=sats, seed=61)
    engine.ring_create(1, 2, n)
    engine.set_channels([gc.Channel(p, dtype=2, f_if=0.0) for p in PRNS])
    engine.loop_set([engine.loop_state(i, 0.0) for i in range(2)])
    engine.rx_start(30)
    retry = int(30 * 1e-3 * 16.368e6)
    hist, pos = [], 0
    frozen = None
    for k, upto in enumerate((40, 80, 100, 120, 140)):
        engine.ring_push_raw(1, sig[pos:upto * NS], upto * NS - pos)
        pos = upto * NS
        engine.rx_step(60)
        hist.append(_record(engine, 60, (1,)))
        st = hist[-1]["status"][0]
        if k < 2:
            assert st["state"] == gc.CH_TRACK and st["attempts"] == 1 and hist[-1]["ndone"][0] >= (9 if k == 0 else 38), (k, st)
        if k == 1:
            engine.rx_set(0, gc.CH_SEARCH)
            assert engine.rx_status()[0]["next_try"] == pos
            frozen = (bytes(engine.loop_get()[0]), engine.trk_get_state()[0])
        if k >= 2:
            assert (bytes(engine.loop_get()[0]), engine.trk_get_state()[0]) == frozen, k
            assert st["state"] == gc.CH_SEARCH and hist[-1]["ndone"][0] == 0 and not np.any(hist[-1]["II"][0]), (k, st)
    s2, s3, s4 = (hist[k]["status"][0] for k in (2, 3, 4))
    assert (s2["attempts"], s2["acq_wrpos"], s2["next_try"]) == (2, 100 * NS, 100 * NS + retry), s2
    assert (s3["attempts"], s3["acq_wrpos"], s3["next_try"], s3["acq"]) == (2, 100 * NS, 100 * NS + retry, s2["acq"]), s3
    assert (s4["attempts"], s4["acq_wrpos"], s4["next_try"]) == (3, 140 * NS, 140 * NS + retry), s4
    ring = orc.make_ring(sig, n, 0)
    for st, wp in ((s2, 100 * NS), (s4, 140 * NS)):
        o = orc.make_chan(PRNS[0], dtype=2, f_if=0.0)
        b, iters = rc.oracle_search(orc, o, ring, wp)
        a = st["acq"]
        assert o.flagacq == 0 and a["flagacq"] == 0 and a["iters"] == iters == 10 and a["buffloc"] == b, (a, o.acq.peakr)
        assert a["acqcodei"] == o.acq.acqcodei and a["freqi"] == o.acq.freqi and a["acqfreq"] == o.acq.acqfreq, a
        assert abs(a["peakr"] - o.acq.peakr) <= 1e-4 * o.acq.peakr and abs(a["cn0"] - o.acq.cn0) <= 1e-4 * abs(o.acq.cn0), a
    o = orc.make_chan(PRNS[1], dtype=2, f_if=0.0)
    attempts, track_steps, periods = _replay(gc, orc, o, ring, 1, hist, 1, 11 * NS, retry, 60, 1e-14, PRNS[1])
    assert attempts == 1 and track_steps == list(range(5)) and all(abs(a - b) <= 1 for a, b in zip(periods[1:], [40, 20, 20, 20])), periods


def test_schedule_across_2_32(gc, orc, synth, engine):
    """The ring's write position is taken to 24.5 code periods below 2^32 (ring_commit by multiples of the ring, as
    tests/test_gpu_positions.py); the ring holds noise there, so both searches of the first step fail below 2^32 and
    their next_try = wp + 30 ms lies above it.  Then 40 periods with PRN 5 arrive: the second step searches a window
    that lies wholly above 2^32, acquires PRN 5 there and tracks it; a third step tracks 15 periods more.  Searches,
    next_try and every tracked period as the oracle's on the same ring."""
    from test_gpu_positions import high_layout, high_ring
    T = 1 << 32
    R, K = high_layout(T, 70 * NS, 8, -25 * NS, -24 * NS)
    D = np.clip(np.rint(np.random.default_rng(71).normal(0.0, 8.0, (R, 2))), -127, 127).astype(np.int8)
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in PRNS}
    new = synth.make_if(codes, 55 * NS, f_sf=16.368e6, f_if=0.0, dtype=2, seed=72,
                        sats=[dict(prn=PRNS[0], doppler=DOP[0], codephase=CPH[0], cn0=47.0, phase=0.3)])
    wp0 = high_ring(engine, 1, 2, D, R, K)
    engine.set_channels([gc.Channel(p, dtype=2, f_if=0.0) for p in (PRNS[0], 9)])
    assert T - 25 * NS <= wp0 <= T - 24 * NS and wp0 % R == 0
    engine.loop_set([engine.loop_state(i, 0.0) for i in range(2)])
    engine.rx_start(30)
    retry = int(30 * 1e-3 * 16.368e6)
    buf = D.copy()
    hist, pos = [], 0
    for upto in (0, 40, 55):
        if upto:
            engine.ring_push_raw(1, new[pos:upto * NS], upto * NS - pos)
            buf[pos:upto * NS] = new[pos:upto * NS]
            pos = upto * NS
        engine.rx_step(30)
        hist.append(_record(engine, 30, (1,)))
    assert [h["wp"][0] for h in hist] == [wp0, wp0 + 40 * NS, wp0 + 55 * NS] and hist[1]["wp"][0] - 11 * NS > T
    for i in range(2):
        s = hist[0]["status"][i]
        assert s["state"] == gc.CH_SEARCH and s["acq_wrpos"] == wp0 < T < s["next_try"] == wp0 + retry <= wp0 + 40 * NS, s
    ring = orc.make_ring(buf, R, 0)
    for i, p in enumerate((PRNS[0], 9)):
        o = orc.make_chan(p, dtype=2, f_if=0.0)
        attempts, track_steps, periods = _replay(gc, orc, o, ring, 1, hist, i, 11 * NS, retry, 30, 1e-14, p)
        assert attempts == 2, (p, attempts)
        if i == 0:
            s = hist[1]["status"][0]
            assert s["state"] == gc.CH_TRACK and s["acq"]["buffloc"] > T and abs(s["acq"]["acqfreq"] - DOP[0]) <= 200.0, s
            assert track_steps == [1, 2] and 9 <= periods[0] <= 10 and 14 <= periods[1] <= 16, periods
        else:
            assert track_steps == [] and hist[2]["status"][1]["next_try"] == wp0 + 40 * NS + retry
