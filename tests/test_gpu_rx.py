"""Receiver schedule on the device (-m gpu): acquisition over a channel list, the device hand-over into the closed
loop, and gnsscorr_rx_step's per-channel state machine (sdrthread(), ref src/sdrmain.c:247-316) against the CPU
oracle.  tests/test_rx_host.py shows on the oracle alone what the cold-start scenario decides."""
import ctypes as C

import numpy as np
import pytest

import rx_cases as rc
from test_gpu_loop import _adopt, _check_against_oracle, _signal

pytestmark = pytest.mark.gpu
F_SF = 16.368e6
NS = 16368
ZERO_RES = dict(acqcodei=0, freqi=0, acqfreq=0.0, cn0=0.0, peakr=0.0, flagacq=0, iters=0, buffloc=0)


# ---- 1. subset = full --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,f_if", [(2, 0.0), (1, 4.092e6)])
def test_acq_subset_equals_full(gc, synth, engine, dtype, f_if):
    """Eight channels on two frequency grids -- seven L1 C/A on ring 1 (int8 IQ at zero IF / real samples at 4.092 MHz),
    one GLONASS G1 on ring 2 -- searched as a whole and as lists of one channel, of three spanning both grids and of all
    in another order, at one write position: a listed channel's result and power array bit for bit the full run's,
    the other rows zero, their power array refused."""
    prns = [3, 7, 11, 14, 20, 26, 31]
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in prns}
    rng = np.random.default_rng(50 + dtype)
    sats = [dict(prn=p, doppler=float(rng.uniform(-4500, 4500)), codephase=float(rng.uniform(0, 1023)), cn0=47.0,
                 phase=float(rng.uniform(0, 6.28))) for p in (3, 20, 31)]
    n = 16 * 16384
    data = synth.make_if(codes, n, f_sf=F_SF, f_if=f_if, dtype=dtype, sats=sats, seed=50 + dtype)
    data2 = rng.integers(-40, 41, size=(n, 2), dtype=np.int8)
    engine.ring_create(1, dtype, n)
    engine.ring_create(2, 2, n)
    engine.ring_push_raw(1, data, n)
    engine.ring_push_raw(2, data2, n)
    chans = [gc.Channel(p, dtype=dtype, f_if=f_if) for p in prns]
    chans.insert(5, gc.Channel(1, ctype=gc.CTYPE_G1, dtype=2, ftype=2, f_if=0.0))
    engine.set_channels(chans)
    wrpos = 14 * NS + 777
    engine.acq_run(wrpos)
    full = engine.acq_fetch()
    assert [r["flagacq"] for r in full] == [1, 0, 0, 0, 1, 0, 0, 1]
    assert all(r["iters"] >= 1 for r in full)
    pfull = {0: engine.acq_power(0), 5: engine.acq_power(5)}
    for chosen in ([4], [5], [0, 5, 7], [7, 6, 5, 4, 3, 2, 1, 0]):
        engine.acq_run(wrpos, channels=chosen)
        sub = engine.acq_fetch()
        for i in range(len(chans)):
            assert sub[i] == (full[i] if i in chosen else ZERO_RES), (chosen, i, sub[i], full[i])
        for i in pfull:
            if i in chosen:
                assert np.array_equal(engine.acq_power(i), pfull[i]), (chosen, i)
            else:
                with pytest.raises(gc.GnsscorrError):
                    engine.acq_power(i)
    # the full run again, after the lists
    engine.acq_run(wrpos)
    assert engine.acq_fetch() == full
    for bad in ([], [0, 0], [8], [-1]):
        with pytest.raises(gc.GnsscorrError):
            engine.acq_run(wrpos, channels=bad)


# ---- 2. device hand-over = host hand-over ----------------------------------------------------------------------------
def test_device_handover_equals_host_handover(gc, synth, engine):
    """After a search over a list, one engine hands over on the device (gnsscorr_loop_start_from_acq), a second through
    the host (acq_fetch -> loop_state -> loop_set -> trk_start_from_acq): loop state and tracking state of every
    channel bit for bit equal -- the acquired ones reset, the failed and the unlisted one untouched -- and so are 200
    closed-loop periods from there."""
    prns, dop, cph = [5, 12, 25, 30], [1517.0, -3222.0, 4630.0, -120.0], [311.3, 12.8, 870.1, 555.5]
    sig = _signal(gc, synth, prns[:3], dop[:3], cph[:3], 222)               # PRN 30 is absent
    n = sig.shape[0]
    listed = [0, 1, 3]                                                      # channel 2 (present) is not searched
    wrpos = 14 * NS

    def prepare(e):
        e.ring_create(1, 2, n)
        e.ring_push_raw(1, sig, n)
        e.set_channels([gc.Channel(p, dtype=2, f_if=0.0) for p in prns])
        # states a running receiver would hold; the channels the hand-over will reset (0, 1): every running field non-zero
        e.trk_set_state([dict(carrfreq=900.0 + i, codefreq=1.023e6 + 0.25 * i, remcode=0.125 * (i + 1), remcarr=0.5 + i,
                              buffloc=3000 + 17 * i) for i in range(4)])
        loops = []
        for i in range(4):
            ls = e.loop_state(i, 800.0 + i, flagsync=1, synci=3 + i, cnt=4000 + i)
            if i >= 2:
                loops.append(ls)
                continue
            ls.navcnt, ls.swloop, ls.carrNco, ls.codeNco, ls.carrErr, ls.codeErr, ls.freqErr = 7, 1, 1.5, -0.25, 0.1, 0.2, 0.3
            ls.biti, ls.bit, ls.swsync, ls.swreset, ls.flagpol, ls.bitIP = 5, -1, 1, 1, 1, 123.0
            for k in range(5):
                ls.II[k], ls.QQ[k], ls.oldI[k], ls.oldQ[k] = 10.0 + k, 20.0 + k, 30.0 + k, 40.0 + k
                ls.sumI[k], ls.sumQ[k], ls.oldsumI[k], ls.oldsumQ[k] = 50.0 + k, 60.0 + k, 70.0 + k, 80.0 + k
            for k in range(20):
                ls.bitsync[k] = k
            loops.append(ls)
        e.loop_set(loops)
        e.acq_run(wrpos, channels=listed)

    host = gc.Engine(0)
    try:
        prepare(engine)
        prepare(host)
        before_loop = [bytes(x) for x in engine.loop_get()]
        before_trk = engine.trk_get_state()
        engine.loop_start_from_acq()
        res = host.acq_fetch()
        assert [r["flagacq"] for r in res] == [1, 1, 0, 0]
        for i, r in enumerate(res):
            if r["flagacq"]:
                host.loop_set([host.loop_state(i, r["acqfreq"])], ch0=i)
        host.trk_start_from_acq()
        dl, hl = engine.loop_get(), host.loop_get()
        dt, ht = engine.trk_get_state(), host.trk_get_state()
        for i in range(4):
            assert bytes(dl[i]) == bytes(hl[i]) and dt[i] == ht[i], i
            if i in (2, 3):
                assert bytes(dl[i]) == before_loop[i] and dt[i] == before_trk[i], i
            else:
                assert dl[i].acqfreq == res[i]["acqfreq"] and dl[i].cnt == 0 and dl[i].flagsync == 0 and dl[i].prn == prns[i]
                assert dt[i] == dict(carrfreq=res[i]["acqfreq"], codefreq=1.023e6, remcode=0.0, remcarr=0.0, buffloc=res[i]["buffloc"])
        engine.trk_run_loop(200)
        host.trk_run_loop(200)
        for a, b in zip(engine.trk_fetch() + engine.trk_fetch_log(), host.trk_fetch() + host.trk_fetch_log()):
            assert a.tobytes() == b.tobytes()
        assert np.all(engine.trk_fetch_log()[1][:2] == 200)
        assert [bytes(x) for x in engine.loop_get()] == [bytes(x) for x in host.loop_get()]
        assert engine.trk_get_state() == host.trk_get_state()
    finally:
        host.close()


# ---- 3 / 4. cold start ------------------------------------------------------------------------------------------------
def _run_schedule(gc, eng, sig, prns):
    """The scenario's pushes and steps on one engine; per step the write position, the status and the tracking part."""
    eng.ring_create(1, 2, 2 * rc.CHUNK)
    eng.set_channels([gc.Channel(p, dtype=2, f_if=0.0) for p in prns])
    eng.loop_set([eng.loop_state(i, 0.0) for i in range(len(prns))])
    eng.rx_start(rc.RETRY_MS)
    st0 = eng.rx_status()
    assert all(s["state"] == gc.CH_SEARCH and s["attempts"] == 0 and s["next_try"] == rc.FIRST_TRY for s in st0)
    hist = []
    for k in range(rc.NCHUNK):
        eng.ring_push_raw(1, sig[k * rc.CHUNK:(k + 1) * rc.CHUNK], rc.CHUNK)
        eng.rx_step(rc.MAX_PERIODS)
        II, QQ, ns = eng.trk_fetch()
        log, ndone = eng.trk_fetch_log()
        hist.append(dict(wp=eng.ring_wrpos(1), status=eng.rx_status(), II=II, QQ=QQ, ns=ns, log=log, ndone=ndone,
                         lapped=eng.trk_loop_lapped()))
    return hist


@pytest.fixture(scope="module")
def cold_start(gc, synth):
    sig = rc.signal(gc, synth)
    out = {"sig": sig}
    for name, prns in (("all", rc.PRNS), ("alone", [rc.PRNS[0]])):
        eng = gc.Engine(0)
        try:
            out[name] = _run_schedule(gc, eng, sig, prns)
        finally:
            eng.close()
    return out


def test_cold_start_against_oracle(gc, orc, cold_start):
    """Six channels, three PRNs present, two absent, one rising after 1 s: the recorded schedule replayed through the
    oracle channel by channel -- orc_sdracquisition on a ring with the search's write position, then
    orc_sdrthread_step with test_gpu_loop's frequency adoption.  Acquisition integers exact, its floats to 1e-4;
    currnsamp, II / QQ, remainders, filter flags, flagsync and navbit of every tracked period exact; the status history
    as the schedule predicts."""
    sig, hist = cold_start["sig"], cold_start["all"]
    L = orc.lib()
    n = sig.shape[0]
    assert [h["wp"] for h in hist] == rc.step_wrpos()
    assert all(h["lapped"] == 0 for h in hist)
    expected_attempts = {p: 1 for p in rc.PRESENT}
    expected_attempts.update({p: 3 for p in rc.ABSENT})
    expected_attempts[rc.LATE] = 2
    for i, p in enumerate(rc.PRNS):
        ring = orc.make_ring(sig, n, 0)
        o = orc.make_chan(p, dtype=2, f_if=0.0)
        state, next_try, attempts = gc.CH_SEARCH, rc.FIRST_TRY, 0
        buffloc = C.c_uint64(0)
        track_steps = []
        for k, h in enumerate(hist):
            wp, st = h["wp"], h["status"][i]
            if state == gc.CH_SEARCH and wp >= next_try:
                attempts += 1
                b, iters = rc.oracle_search(orc, o, ring, wp)
                a = st["acq"]
                where = (p, k, a, o.acq.peakr)
                assert st["attempts"] == attempts and st["acq_wrpos"] == wp, where
                assert a["flagacq"] == o.flagacq and a["iters"] == iters and a["buffloc"] == b, where
                assert a["acqcodei"] == o.acq.acqcodei and a["freqi"] == o.acq.freqi and a["acqfreq"] == o.acq.acqfreq, where
                assert abs(a["peakr"] - o.acq.peakr) <= 1e-4 * o.acq.peakr, where
                assert abs(a["cn0"] - o.acq.cn0) <= 1e-4 * abs(o.acq.cn0), where
                if o.flagacq:
                    state = gc.CH_TRACK
                    buffloc.value = b
                else:
                    next_try = wp + rc.RETRY_SAMPLES
            assert st["state"] == state and st["attempts"] == attempts, (p, k, st)
            if state == gc.CH_SEARCH:
                assert st["next_try"] == next_try, (p, k, st)
            II, QQ, ns, log, ndone = h["II"][i], h["QQ"][i], h["ns"][i], h["log"][i], int(h["ndone"][i])
            e = 0
            if state == gc.CH_TRACK:
                track_steps.append(k)
                ring.wrpos = wp
                while e < rc.MAX_PERIODS and L.orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(buffloc)):
                    where = (p, k, e)
                    assert ns[e] == o.currnsamp and log[e]["currnsamp"] == o.currnsamp, where
                    assert np.array_equal(II[e], np.ctypeslib.as_array(o.II)[:5]), where
                    assert np.array_equal(QQ[e], np.ctypeslib.as_array(o.QQ)[:5]), where
                    r = log[e]
                    assert r["flagloopfilter"] == o.flagloopfilter, where
                    assert r["remcode"] == o.remcode and r["remcarr"] == o.remcarr, where
                    _adopt(o, r, where)
                    e += 1
                if k > track_steps[0]:
                    assert e >= rc.CHUNK // NS - 1, (p, k, e)           # the channel keeps up with the stream
                assert st["cnt"] == o.cnt, (p, k)
            assert ndone == e, (p, k, ndone, e)
            assert np.all(ns[e:] == 0) and not np.any(II[e:]) and not np.any(QQ[e:]), (p, k)
            assert log[e:].tobytes() == bytes(log[e:].nbytes), (p, k)
        assert attempts == expected_attempts[p], (p, attempts)
        if p in rc.PRESENT:
            assert track_steps == list(range(rc.NCHUNK)), p
            if p > 5:                                                   # (checksync()'s shift-register branch, ref src/sdrnav.c:203)
                assert o.flagsync == 1, p                               # 3.5 s: through bit synchronisation into the 10-period loop
            assert abs(o.carrfreq - rc.PRESENT[p][0]) < 30.0, (p, o.carrfreq)
        elif p in rc.ABSENT:
            assert track_steps == [] and state == gc.CH_SEARCH, p
        else:
            assert track_steps == list(range(6, rc.NCHUNK)), p          # only after its retry
            assert abs(o.carrfreq - rc.LATE_DOPPLER) < 30.0, o.carrfreq


def test_cold_start_tracking_channel_is_not_disturbed(cold_start):
    """A channel acquired at the first search, in the six-channel run and alone on a second engine with the same
    pushes: its tracking outputs bit for bit the same in every step, those in which other channels were searched
    (steps 6 and 12) included."""
    searched = [k for k, h in enumerate(cold_start["all"])
                if any(s["acq_wrpos"] == h["wp"] for s in h["status"][1:])]
    assert searched == [0, 6, 12]
    for k, (a, b) in enumerate(zip(cold_start["all"], cold_start["alone"])):
        assert a["ndone"][0] == b["ndone"][0] > 0, k
        assert a["log"][0].tobytes() == b["log"][0].tobytes(), k
        for f in ("II", "QQ", "ns"):
            assert a[f][0].tobytes() == b[f][0].tobytes(), (k, f)
        assert a["status"][0] == b["status"][0], k


# ---- 5. parking -------------------------------------------------------------------------------------------------------
def test_parking_freezes_and_search_rearms(gc, synth, engine):
    """rx_set(ch, IDLE) on a tracking channel: its tracking and loop state stay bit for bit over later steps, it plans
    no period, the other channel goes on; rx_set(ch, SEARCH) makes it due at the current write position, and the next
    step acquires it again."""
    prns = [5, 12]
    chunk = 40 * NS
    sig = _signal(gc, synth, prns, [1517.0, -3222.0], [311.3, 12.8], 200)
    engine.ring_create(1, 2, 2 * chunk)
    engine.set_channels([gc.Channel(p, dtype=2, f_if=0.0) for p in prns])
    engine.loop_set([engine.loop_state(i, 0.0) for i in range(2)])
    with pytest.raises(gc.GnsscorrError):
        engine.rx_set(0, gc.CH_IDLE)                                    # no schedule yet
    engine.rx_start()
    with pytest.raises(gc.GnsscorrError):
        engine.rx_set(0, gc.CH_TRACK)

    def push_step(k):
        engine.ring_push_raw(1, sig[k * chunk:(k + 1) * chunk], chunk)
        engine.rx_step(60)
        return engine.trk_fetch_log()[1], engine.rx_status()

    ndone, st = push_step(0)
    assert [s["state"] for s in st] == [gc.CH_TRACK] * 2 and np.all(ndone >= 9)
    engine.rx_set(0, gc.CH_IDLE)
    frozen = (bytes(engine.loop_get()[0]), engine.trk_get_state()[0])
    for k in (1, 2):
        ndone, st = push_step(k)
        assert ndone[0] == 0 and ndone[1] >= 39, (k, ndone)
        assert st[0]["state"] == gc.CH_IDLE and st[0]["attempts"] == 1 and st[1]["state"] == gc.CH_TRACK
        assert (bytes(engine.loop_get()[0]), engine.trk_get_state()[0]) == frozen, k
        II, QQ, ns = engine.trk_fetch()
        assert not np.any(II[0]) and not np.any(QQ[0]) and not np.any(ns[0])
    engine.rx_set(0, gc.CH_SEARCH)
    st = engine.rx_status()
    assert st[0]["state"] == gc.CH_SEARCH and st[0]["next_try"] == engine.ring_wrpos(1) == 3 * chunk
    assert (bytes(engine.loop_get()[0]), engine.trk_get_state()[0]) == frozen
    ndone, st = push_step(3)
    assert st[0]["state"] == gc.CH_TRACK and st[0]["attempts"] == 2 and st[0]["acq_wrpos"] == 4 * chunk
    assert st[0]["acq"]["flagacq"] == 1 and abs(st[0]["acq"]["acqfreq"] - 1517.0) <= 200.0
    assert ndone[0] >= 9 and ndone[1] >= 39 and st[0]["cnt"] == ndone[0]
    assert engine.trk_get_state()[0]["buffloc"] > 3 * chunk


# ---- 6. opt-in --------------------------------------------------------------------------------------------------------
def test_engine_without_rx_start_behaves_as_before(gc, orc, synth, engine):
    """No gnsscorr_rx_start: the schedule's entry points refuse, acq_run searches every channel and trk_run_loop tracks
    every channel, against the oracle (one present PRN, one absent: the absent one is tracked on noise, as before)."""
    prns = [5, 9]
    sig = _signal(gc, synth, [5], [1517.0], [311.3], 60)
    n = sig.shape[0]
    engine.ring_create(1, 2, n)
    engine.ring_push_raw(1, sig, n)
    engine.set_channels([gc.Channel(p, dtype=2, f_if=0.0) for p in prns])
    for call in (lambda: engine.rx_step(10), engine.rx_status):
        with pytest.raises(gc.GnsscorrError):
            call()
    wrpos = 14 * NS
    engine.acq_run(wrpos)
    res = engine.acq_fetch()
    ring = orc.make_ring(sig, n, wrpos)
    ochs, bufflocs = [], []
    for i, p in enumerate(prns):
        o = orc.make_chan(p, dtype=2, f_if=0.0)
        b, iters = rc.oracle_search(orc, o, ring, wrpos)
        r = res[i]
        assert r["flagacq"] == o.flagacq == (1 if p == 5 else 0) and r["iters"] == iters and r["buffloc"] == b
        assert r["acqcodei"] == o.acq.acqcodei and r["freqi"] == o.acq.freqi and r["acqfreq"] == o.acq.acqfreq
        assert abs(r["peakr"] - o.acq.peakr) <= 1e-4 * o.acq.peakr
        if not o.flagacq:                                               # hand-set, as callers without a schedule do
            o.carrfreq, o.codefreq, b = 1000.0, o.crate, 5000
            engine.trk_set_state([dict(carrfreq=1000.0, codefreq=o.crate, remcode=0.0, remcarr=0.0, buffloc=b)], ch0=i)
        o.acq.acqfreq = r["acqfreq"]
        ochs.append(o)
        bufflocs.append(C.c_uint64(b))
    engine.trk_start_from_acq()
    engine.loop_set([engine.loop_state(i, res[i]["acqfreq"]) for i in range(2)])
    ring.wrpos = n
    ndone = _check_against_oracle(orc, engine, ochs, ring, bufflocs, 40, 5)
    assert np.all(ndone == 40)
