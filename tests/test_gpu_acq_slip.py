"""Code-Doppler compensation across the groups of a search (gnsscorr_acq_set_codedoppler) on the device against the
restatement of its semantics (tests/acq_slip_cases.py; parity tests proper, -m gpu).  tests/test_acq_slip_host.py shows
on the host that every scenario here is decided with room.

Bars, those of tests/test_gpu_acq_coherent.py: flagacq, iters, buffloc, acqcodei, freqi and acqfreq (and the bit edge)
identical to the restatement's; peakr and cn0 to 1e-4; the device's cn0 within 1e-9 of checkacquisition()'s formula over
its own power array and ncoh*ctime; acq_power element-wise, |P_gpu - P_td| <= acq_cases.POWER_TOL x (the Doppler row's
mean outside the exclusion window), P_td the fp64 time-domain sum over the same groups from the same shifted starts
(acq_slip_cases.slip_power_td).  The shift tables are equal to the restatement's integer by integer.

Measured on the MI355X (every check prints its ratio and the largest so far): the largest was 1.4e-5
(`m20`, 40 dB-Hz on the 65536-point path; 1.3e-5 for `drift`'s compensated channel); 0.3e-5 to 1.0e-5 for the other
channels, groups of 5 and of 20 alike.  The file runs in about 3 s."""
import ctypes as C

import numpy as np
import pytest

import acq_cases as ac
import acq_coh_cases as cc
import acq_slip_cases as sl
from test_gpu_loop import _adopt

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
_ratios = []


def _granule(n, dtype):
    g = 16 // dtype
    return -(-n // g) * g


def _load(engine, sc, W, ftype=1):
    ringlen = _granule(len(W), sc["dtype"])
    engine.ring_create(ftype, sc["dtype"], ringlen)
    engine.ring_push_raw(ftype, W, len(W))
    assert engine.ring_wrpos(ftype) == len(W)
    return ringlen


def _check_results(engine, chans, wants, where=""):
    res = engine.acq_fetch()
    for i, (c, r, w) in enumerate(zip(chans, res, wants)):
        ac.check_result(r, w, (where, i, c.prn, c.ncoh))
    edge = engine.acq_fetch_edge()
    assert edge == [w.get("edge", -1) for w in wants], (where, edge)
    return res


def _check_tables(engine, chans, wants, where=""):
    for i, (c, w) in enumerate(zip(chans, wants)):
        s, back = engine.acq_fetch_shifts(i)
        assert s.dtype == np.int32 and np.array_equal(s, w["shifts"]) and back == w["back"], (where, i, s, back)
    assert engine.acq_get_codedoppler() == [c.f_cf if c.cdop else 0.0 for c in chans]


def _check_power(engine, orc, i, c, o, want, ring, where="", seed=0):
    """acq_power of channel i: shape, the device's cn0 over its own array, and the element-wise bar at the lags of
    acq_cases.check_lags."""
    buf, ringlen = ring
    P = engine.acq_power(i)
    assert P.shape == want["P"].shape
    r = engine.acq_fetch()[i]
    cn0 = ac._cn0_restated(P, r["acqcodei"], r["freqi"], c.nsampchip, c.ncoh * c.ctime)
    assert abs(r["cn0"] - cn0) <= 1e-9 * abs(cn0), (where, i, r["cn0"], cn0)
    lags = ac.check_lags(o, want["acqcodei"], np.random.default_rng(seed + i))
    td = sl.slip_power_td(orc, o, buf, ringlen, want["b0"], want["groups"], c.ncoh, want["shifts"], lags, want.get("hsel"))
    ratio = ac.power_ratio(P, td, lags, want["P"], want["acqcodei"], c.nsampchip)
    _ratios.append(ratio)
    print(f"power {where} ch {i} prn {c.prn} ncoh {c.ncoh} groups {want['groups']} back {want['back']}: "
          f"max |dP|/meanP {ratio:.3g} (largest so far {max(_ratios):.3g})")
    assert ratio <= ac.POWER_TOL, (where, i, ratio)
    return P


def _scenario_on_engine(engine, gc, orc, synth, name, power=()):
    """The scenario as tests/acq_slip_cases.py states it: ring = its span, the search ends at the span's last sample."""
    sc = sl.SCEN[name]
    W, pairs, wants = sl.scenario(gc, orc, synth, name)
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    _load(engine, sc, W)
    engine.set_channels(chans)
    engine.acq_run(len(W))
    _check_tables(engine, chans, wants, name)
    res = _check_results(engine, chans, wants, name)
    for i in power:
        _check_power(engine, orc, i, chans[i], ochs[i], wants[i], (W, len(W)), name)
    return chans, res, wants


# ---- 1. / 2. off, and a table of zeros -------------------------------------------------------------------------------
def _plain_chans(gc, name):
    sc = cc.SCEN[name]
    return sc, [gc.Channel(p, dtype=sc["dtype"], f_sf=sc["f_sf"], f_if=sc["f_if"], hband=h, step=s, intg=i, ncoh=k)
                for p, h, s, i, k in sc["chans"]]


@pytest.mark.parametrize("name", ["iq10", "m20"])
@pytest.mark.parametrize("f_cf", [0.0, 1e30], ids=["zeros", "1e30"])
def test_off_and_zero_shifts_are_bitwise_the_engine_that_never_called_it(gc, synth, engine, name, f_cf):
    """After the setter with all zeros, and with a carrier of 1e30 Hz (every shift 0, back 0: the search goes through the
    compensating instance of acq_fwd and reads a table of zeros), results and power arrays are bit for bit those of an
    engine that never called it: groups of 10 and 5 on the 32768-point path, 20 Msps on the 65536-point one."""
    sc, chans = _plain_chans(gc, name)
    W = cc.make_span(gc, synth, sc)
    other = gc.Engine(0)
    try:
        out = []
        for e, call in ((engine, False), (other, True)):
            _load(e, sc, W)
            e.set_channels(chans)
            assert e.acq_get_codedoppler() == [0.0] * len(chans)
            if call:
                e.acq_set_codedoppler([f_cf] * len(chans))
                assert e.acq_get_codedoppler() == [f_cf] * len(chans)
                assert e.acq_get_coherent() == [c.ncoh for c in chans]          # (the other settings stay)
            e.acq_run(len(W))
            for i in range(len(chans)):
                s, back = e.acq_fetch_shifts(i)
                assert not s.any() and back == 0 and s.shape == (chans[i].nfreq, chans[i].intg // chans[i].ncoh)
            out.append((e.acq_fetch(), [e.acq_power(i).tobytes() for i in range(len(chans))]))
        assert out[0][0] == out[1][0]
        assert out[0][1] == out[1][1]
        assert all(r["iters"] > 0 for r in out[0][0]) and (chans[0].nsamp > 16384) == (name == "m20")
    finally:
        other.close()


# ---- 3. the scenarios ------------------------------------------------------------------------------------------------
def test_drift_needs_the_compensation(gc, orc, synth, engine):
    """The satellite of the host test, two channels on its PRN in one engine: without compensation it passes at no
    group, with it at group 4, at the placed lag -- the lag of group 0's frame, which buffloc hands over."""
    chans, res, wants = _scenario_on_engine(engine, gc, orc, synth, "drift", power=(0, 1))
    assert [c.cdop for c in chans] == [True, False]
    assert res[0]["flagacq"] and res[0]["acqcodei"] == 1234 and res[0]["buffloc"] == 1234 and res[0]["iters"] == 25
    assert not res[1]["flagacq"] and res[1]["iters"] == 40 and res[1]["buffloc"] == 3 + 40 * 4092
    print("drift: compensated peakr %.3f cn0 %.2f; uncompensated peakr %.3f cn0 %.2f"
          % (res[0]["peakr"], res[0]["cn0"], res[1]["peakr"], res[1]["cn0"]))


def test_negative_doppler_looks_further_back(gc, orc, synth, engine):
    """back = 3: the satellite in the lowest bin, whose groups start later, and an absent PRN through all eight groups."""
    chans, res, wants = _scenario_on_engine(engine, gc, orc, synth, "neg", power=(0, 1))
    assert wants[0]["back"] == 3 and res[0]["flagacq"] and res[0]["freqi"] == 0 and not res[1]["flagacq"]


def test_negative_doppler_search_ends_at_a_wrapped_position(gc, orc, synth, engine):
    """`neg` in a ring of 43 periods that ends 7.5 periods into the span (inside group 1), the stream pushed in pieces:
    the same samples, the same search, ending past the ring's length."""
    sc = sl.SCEN["neg"]
    W, pairs, ref = sl.scenario(gc, orc, synth, "neg")
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    n = chans[0].nsamp
    ringlen = _granule(43 * n, 2)
    b0 = ringlen - (7 * n + n // 2)
    wrpos = b0 + len(W)
    stream = np.concatenate([ac.noise(b0, 2, 77), W])
    engine.ring_create(1, 2, ringlen)
    ac.push_wrapping(engine, 1, stream, wrpos, ringlen)
    assert engine.ring_wrpos(1) == wrpos > ringlen
    engine.set_channels(chans)
    buf = ac.ring_order(stream, ringlen, wrpos)
    wants = sl.restate(orc, pairs, sc["chans"], buf, ringlen, wrpos)
    for w, r in zip(wants, ref):
        assert w["b0"] == b0 and w["steps"] == r["steps"] and w["buffloc"] == r["buffloc"] + b0
    engine.acq_run(wrpos)
    _check_tables(engine, chans, wants, "wrap")
    _check_results(engine, chans, wants, "wrap")
    _check_power(engine, orc, 0, chans[0], ochs[0], wants[0], (buf, ringlen), "wrap")
    engine.acq_run(0)                                       # the ring's own write position: the same search
    _check_results(engine, chans, wants, "wrap, wrpos 0")


def test_l1_carrier_200_periods(gc, orc, synth, engine):
    """The real constant: f_cf 1575.42 MHz, intg 200 in ten groups of 20, bins at -5, 0 and +5 kHz, shifts up to +-2."""
    chans, res, wants = _scenario_on_engine(engine, gc, orc, synth, "l1", power=(1, 2))
    assert [c.f_cf for c in chans] == [1575.42e6] * 3 and wants[0]["shifts"].min() == -2 and wants[0]["back"] == 2
    assert [r["flagacq"] for r in res] == [1, 1, 0] and res[2]["iters"] == 200


def test_with_bit_edge_hypotheses(gc, orc, synth, engine):
    """drift's shape with every hypothesis (estep 1, H = 5: acq_fwd's EDGE instance with the table, the table indexed by
    the group, not the slot); the group with the flipped bit chooses h = 2."""
    chans, res, wants = _scenario_on_engine(engine, gc, orc, synth, "edge", power=(0,))
    assert chans[0].estep == 1 and engine.acq_get_bitedge() == [1] and res[0]["flagacq"] and res[0]["iters"] > 10


def test_65536_point_path(gc, orc, synth, engine):
    """20 Msps, nsamp 20000, 9 bins, intg 8, ncoh 2: the four-residue transform from shifted origins, back = 12."""
    chans, res, wants = _scenario_on_engine(engine, gc, orc, synth, "m20", power=(0,))
    assert chans[0].nsamp == 20000 and wants[0]["back"] == 12 and res[0]["flagacq"] and res[0]["iters"] == 4


# ---- 4. mixed grids: lists, subsets, repeats -------------------------------------------------------------------------
def test_mixed_carriers_full_list_subsets_and_repeat(gc, orc, synth, engine):
    """One ring, five channels: two carriers, none (twice), and the first carrier again on another PRN -- three sets of
    forward spectra with back 3, 2 and 0, the two uncompensated channels and channels 0 / 4 sharing theirs.  Run as the
    full list, repeated, and as subsets on an engine whose buffers are poisoned (a subset without a compensated grid
    runs the plain instance): a listed channel's result and power array are bit for bit the same in all of them."""
    sc = sl.SCEN["mixed"]
    W, pairs, wants = sl.scenario(gc, orc, synth, "mixed")
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    _load(engine, sc, W)
    engine.set_channels(chans)
    engine.acq_run(len(W))
    _check_tables(engine, chans, wants, "mixed")
    full = _check_results(engine, chans, wants, "mixed")
    assert all(r["flagacq"] for r in full)
    assert [r["buffloc"] - r["acqcodei"] for r in full] == [0, 1, 3, 3, 0]       # b0 = 3 - back
    N = len(chans)
    Pfull = [engine.acq_power(i).tobytes() for i in range(N)]
    for i in (0, 1, 2):
        _check_power(engine, orc, i, chans[i], ochs[i], wants[i], (W, len(W)), "mixed")
    engine.acq_run(len(W))                                  # repeated over the same list
    assert engine.acq_fetch() == full
    assert [engine.acq_power(i).tobytes() for i in range(N)] == Pfull
    other = gc.Engine(0)
    try:
        other.debug_poison(0xA5)
        _load(other, sc, W)
        other.set_channels(chans)
        for sub in ([1], [3, 2], [4, 0], [2, 1, 4], [0]):
            other.acq_run(len(W), channels=sub)
            res = other.acq_fetch()
            for i in range(N):
                if i in sub:
                    assert res[i] == full[i], (sub, i)
                    assert other.acq_power(i).tobytes() == Pfull[i], (sub, i)
                else:
                    assert res[i]["flagacq"] == 0 and res[i]["iters"] == 0, (sub, i)
    finally:
        other.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_refusals(gc, orc, synth, engine):
    """ESTATE while the ring holds fewer than (intg + 1) n + back samples (one more sample and the search runs), EINVAL
    for a ring shorter than that, for the setter's bad arguments (nothing touched), and at prepare for a shift beyond a
    code period; fetch_shifts refuses before the first prepare."""
    sc = sl.SCEN["drift"]
    W, pairs, wants = sl.scenario(gc, orc, synth, "drift")
    chans = [c for c, _ in pairs]
    L = gc.lib()
    need = 41 * 4092 + 3
    assert len(W) == need and wants[0]["back"] == 3
    with pytest.raises(gc.GnsscorrError):
        engine.acq_set_codedoppler([sl.F41])                # no channels yet
    engine.ring_create(1, 2, _granule(need, 2))
    engine.ring_push_raw(1, W[:need - 1], need - 1)
    engine.set_channels(chans[:1])
    s = np.zeros((5, 8), np.int32)
    back = C.c_int(-1)
    assert L.gnsscorr_acq_fetch_shifts(engine.h, 0, s.ctypes.data, C.byref(back)) == ESTATE     # nothing prepared yet
    assert L.gnsscorr_acq_run(engine.h, 0) == ESTATE
    assert "%d needed" % need in L.gnsscorr_last_error().decode()
    assert L.gnsscorr_acq_run(engine.h, need - 1) == ESTATE
    engine.ring_push_raw(1, W[need - 1:], 1)
    engine.acq_run(0)
    _check_results(engine, chans[:1], wants[:1], "after ESTATE")
    before = engine.acq_fetch()
    bad = [([-1.0], 0), ([float("nan")], 0), ([float("inf")], 0), ([-float("inf")], 0), ([sl.F41, sl.F41], 0),
           ([sl.F41], 1), ([sl.F41], -1), ([], 0)]
    for f_cf, ch0 in bad:
        with pytest.raises(gc.GnsscorrError):
            engine.acq_set_codedoppler(f_cf, ch0=ch0)
        assert engine.acq_get_codedoppler() == [sl.F41], (f_cf, ch0)
    assert L.gnsscorr_acq_set_codedoppler(engine.h, 0, 1, (C.c_double * 1)(-2.5)) == EINVAL
    assert "channel 0" in L.gnsscorr_last_error().decode()
    assert engine.acq_fetch() == before                     # (a refusal does not drop the last search either)
    assert L.gnsscorr_acq_fetch_shifts(engine.h, 1, s.ctypes.data, C.byref(back)) == EINVAL
    # a ring shorter than the look-back with `back`: EINVAL
    short = gc.Engine(0)
    try:
        ringlen = _granule(41 * 4092, 2)                    # holds the 41 periods and drift's back, not a back of 14
        assert 41 * 4092 + 3 <= ringlen < 41 * 4092 + 14
        short.ring_create(1, 2, ringlen)
        short.ring_push_raw(1, W, need)
        short.ring_push_raw(1, W[:19], 19)
        short.set_channels(chans[:1])
        short.acq_set_codedoppler([sl.F41 / 4])
        assert L.gnsscorr_acq_run(short.h, 0) == EINVAL
        assert short.acq_fetch_shifts(0)[1] == 14           # (prepared: the tables are there)
        short.acq_set_codedoppler([0.0])                    # without compensation the ring is long enough
        short.acq_run(0)
    finally:
        short.close()
    # a carrier so small that a shift exceeds a code period: the search that prepares refuses, the setting stays
    engine.acq_set_codedoppler([1000.0 * 35 * 4092 / 4092.4])       # |x| = 4092.4 at the outer bins' last group: allowed
    assert L.gnsscorr_acq_run(engine.h, 0) == ESTATE                # (prepared; the ring would have to hold back = 4092 more)
    assert "%d needed" % (41 * 4092 + 4092) in L.gnsscorr_last_error().decode()
    assert np.abs(engine.acq_fetch_shifts(0)[0]).max() == 4092 == engine.acq_fetch_shifts(0)[1]
    engine.acq_set_codedoppler([1000.0 * 35 * 4092 / 4093.4])       # 4093.4: more than a code period
    with pytest.raises(gc.GnsscorrError):
        engine.acq_fetch()                                  # a change drops the last search
    assert L.gnsscorr_acq_run(engine.h, 0) == EINVAL
    assert "code period" in L.gnsscorr_last_error().decode()
    assert L.gnsscorr_acq_fetch_shifts(engine.h, 0, s.ctypes.data, C.byref(back)) == ESTATE
    engine.acq_set_codedoppler([sl.F41])
    engine.acq_run(0)
    assert engine.acq_fetch() == before
    engine.set_channels([gc.Channel(1, dtype=2, f_sf=4.092e6, hband=1000, step=500, intg=40)])
    assert engine.acq_get_codedoppler() == [0.0]            # set_channels resets; Channel.cdop is off by default


# ---- 6. the receiver schedule ---------------------------------------------------------------------------------------
def test_schedule_waits_for_back_and_tracks_from_the_handover(gc, orc, synth, engine):
    """gnsscorr_rx_start on `drift`'s compensated channel: first due at (intg + 1) n + back samples -- a step one sample
    short of that searches nothing -- then the search of the scenario, the hand-over, and the closed loop's first
    periods against orc_sdrthread_step from the handed-over state (carrfreq = acqfreq, codefreq = crate, buffloc = the
    lag of group 0's frame)."""
    sc = sl.SCEN["drift"]
    W, pairs, wants = sl.scenario(gc, orc, synth, "drift")
    (c, _), w = pairs[0], wants[0]
    n, need = c.nsamp, len(W)
    assert need == 41 * n + w["back"] and w["back"] == 3 and w["flagacq"]
    ringlen = _granule(need, 2)
    engine.ring_create(1, 2, ringlen)
    engine.set_channels([c])
    engine.loop_set([engine.loop_state(0, 0.0)])
    engine.rx_start()
    assert engine.rx_status()[0]["next_try"] == need
    NPER = 5
    engine.ring_push_raw(1, W[:need - 1], need - 1)         # past (intg + 1) n, short of back
    engine.rx_step(NPER)
    st = engine.rx_status()[0]
    assert (st["state"], st["attempts"], st["next_try"]) == (gc.CH_SEARCH, 0, need)
    engine.ring_push_raw(1, W[need - 1:], 1)
    engine.rx_step(NPER)
    st = engine.rx_status()[0]
    assert (st["state"], st["attempts"], st["acq_wrpos"]) == (gc.CH_TRACK, 1, need)
    ac.check_result(st["acq"], w, "rx")
    s, back = engine.acq_fetch_shifts(0)
    assert np.array_equal(s, w["shifts"]) and back == 3
    II, QQ, ns = engine.trk_fetch()
    log, ndone = engine.trk_fetch_log()
    assert ndone[0] == NPER
    buf = np.zeros((ringlen, 2), np.int8)
    buf[:need] = W
    ring = orc.make_ring(buf, ringlen, need)
    o = orc.make_chan(c.prn, dtype=2, f_cf=c.f_cf, f_sf=c.f_sf, f_if=0.0)
    o.acq.acqfreq = w["acqfreq"]
    o.carrfreq, o.codefreq, o.remcode, o.remcarr = w["acqfreq"], c.crate, 0.0, 0.0
    buffloc = C.c_uint64(w["buffloc"])
    for e in range(NPER):
        assert orc.lib().orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(buffloc)) == 1
        assert ns[0, e] == o.currnsamp and log[0, e]["currnsamp"] == o.currnsamp, e
        assert np.array_equal(II[0, e], np.ctypeslib.as_array(o.II)[:5]), e
        assert np.array_equal(QQ[0, e], np.ctypeslib.as_array(o.QQ)[:5]), e
        r = log[0, e]
        assert r["flagloopfilter"] == o.flagloopfilter and r["remcode"] == o.remcode and r["remcarr"] == o.remcarr, e
        _adopt(o, r, e)
    assert engine.rx_status()[0]["cnt"] == o.cnt == NPER
