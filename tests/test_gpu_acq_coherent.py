"""Coherent integration over several code periods per search (gnsscorr_acq_set_coherent) on the device against the
restatement of its semantics (tests/acq_coh_cases.py; parity tests proper, -m gpu).  tests/test_acq_coh_host.py shows on
the host that every scenario here is decided with room.

Bars, those of tests/test_gpu_acq_edges.py::_check: flagacq, iters, buffloc, acqcodei, freqi and acqfreq identical to
the restatement's; peakr and cn0 to 1e-4; the device's cn0 within 1e-9 of checkacquisition()'s formula over its own
power array and ncoh*ctime; acq_power element-wise, |P_gpu - P_td| <= acq_cases.POWER_TOL x (the Doppler row's mean
outside the exclusion window), P_td the fp64 time-domain sum over the same groups (acq_coh_cases.coh_power_td).

Measured on the MI355X (every check prints its ratio and the largest so far): the largest was 6.6e-5, in
test_mixed_ncoh_full_list_subsets_and_repeat (41 dB-Hz, one group of 10 on 201 bins); 3.3e-5 to 3.7e-5 for the other
groups of 10 and of 4, 0.8e-5 to 2.3e-5 for groups of 5 and 2.  The file runs in about 6 s."""
import numpy as np
import pytest

import acq_cases as ac
import acq_coh_cases as cc

pytestmark = pytest.mark.gpu

_ratios = []


def _granule(n, dtype):
    g = 16 // dtype
    return -(-n // g) * g


def _load(engine, sc, W, ftype=1):
    """Ring `ftype` holding the span from sample 0 on: (ring view for the restatement, ringlen, write position)."""
    ringlen = _granule(len(W), sc["dtype"])
    engine.ring_create(ftype, sc["dtype"], ringlen)
    engine.ring_push_raw(ftype, W, len(W))
    assert engine.ring_wrpos(ftype) == len(W)
    return ringlen


def _check_results(engine, chans, wants, where=""):
    res = engine.acq_fetch()
    for i, (c, r, w) in enumerate(zip(chans, res, wants)):
        ac.check_result(r, w, (where, i, c.prn, c.ncoh))
    return res


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
    td = cc.coh_power_td(orc, o, buf, ringlen, want["b0"], want["groups"], c.ncoh, lags)
    ratio = ac.power_ratio(P, td, lags, want["P"], want["acqcodei"], c.nsampchip)
    _ratios.append(ratio)
    print(f"power {where} ch {i} prn {c.prn} ncoh {c.ncoh} groups {want['groups']}: max |dP|/meanP {ratio:.3g} "
          f"(largest so far {max(_ratios):.3g})")
    assert ratio <= ac.POWER_TOL, (where, i, ratio)
    return P


def _scenario_on_engine(engine, gc, orc, synth, name, power=()):
    """The scenario as tests/acq_coh_cases.py states it: ring = its span, the search ends at the span's last sample."""
    sc = cc.SCEN[name]
    W, pairs, wants = cc.scenario(gc, orc, synth, name)
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    _load(engine, sc, W)
    engine.set_channels(chans)
    assert engine.acq_get_coherent() == [c.ncoh for c in chans]
    engine.acq_run(len(W))
    res = _check_results(engine, chans, wants, name)
    for i in power:
        _check_power(engine, orc, i, chans[i], ochs[i], wants[i], (W, len(W)), name)
    return chans, res, wants


# ---- 1. all ones: nothing changes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["iq10", "real", "m20"])
def test_all_ones_is_bitwise_the_engine_that_never_called_it(gc, synth, engine, name):
    """After acq_set_coherent with all ones, results and power arrays are bit for bit those of an engine that never
    called it: IQ and real samples on the 32768-point path, 20 Msps on the 65536-point one."""
    sc = cc.SCEN[name]
    W = cc.make_span(gc, synth, sc)
    chans = [gc.Channel(p, dtype=sc["dtype"], f_sf=sc["f_sf"], f_if=sc["f_if"], hband=h, step=s, intg=i)
             for p, h, s, i, _ in sc["chans"]]
    other = gc.Engine(0)
    try:
        out = []
        for e, call in ((engine, False), (other, True)):
            _load(e, sc, W)
            e.set_channels(chans)
            if call:
                e.acq_set_coherent([1] * len(chans))
                assert e.acq_get_coherent() == [1] * len(chans)
            e.acq_run(len(W))
            out.append((e.acq_fetch(), [e.acq_power(i).tobytes() for i in range(len(chans))]))
        assert out[0][0] == out[1][0]
        assert out[0][1] == out[1][1]
        assert all(r["iters"] > 0 for r in out[0][0]) and (chans[0].nsamp > 16384) == (name == "m20")
    finally:
        other.close()


# ---- 2. groups -----------------------------------------------------------------------------------------------------
def test_groups_of_ten_and_five(gc, orc, synth, engine):
    """IQ, intg 10: one group of 10; groups of 5 for a satellite that passes at group 1, one that passes only at group
    2 (negative Doppler: a falling carrier phase), and an absent PRN (iters = intg, the not-acquired buffloc)."""
    chans, res, wants = _scenario_on_engine(engine, gc, orc, synth, "iq10", power=(0, 1, 2, 3))
    assert [c.ncoh for c in chans] == [10, 5, 5, 5]
    assert [(r["flagacq"], r["iters"]) for r in res] == [(1, 10), (1, 5), (1, 10), (0, 10)]
    n = chans[0].nsamp
    assert res[3]["buffloc"] == 10 * n and res[2]["buffloc"] == res[2]["acqcodei"] == 777 and res[2]["acqfreq"] == -200.0


# ---- 3. the weak satellite -----------------------------------------------------------------------------------------
def test_weak_satellite_two_channels_one_engine(gc, orc, synth, engine):
    """The weak satellite of the host test, two channels on its PRN in one engine: the reference's integration on 71
    bins does not acquire it, one group of 10 ms on 201 bins does, at its lag and bin."""
    chans, res, wants = _scenario_on_engine(engine, gc, orc, synth, "weak", power=(1,))
    assert [(c.ncoh, c.nfreq) for c in chans] == [(1, 71), (10, 201)]
    assert not res[0]["flagacq"] and res[0]["iters"] == 10
    assert res[1]["flagacq"] and res[1]["iters"] == 10 and abs(res[1]["acqcodei"] - 1234) <= 1 and res[1]["freqi"] == 120
    print("weak satellite: ncoh 1 peakr %.3f cn0 %.2f; ncoh 10 peakr %.3f cn0 %.2f"
          % (res[0]["peakr"], res[0]["cn0"], res[1]["peakr"], res[1]["cn0"]))


# ---- 4. mixed grids: lists, subsets, repeats -----------------------------------------------------------------------
def test_mixed_ncoh_full_list_subsets_and_repeat(gc, orc, synth, engine):
    """One engine with ncoh 1 / 5 / 5 / 10 channels on grids of 71 / 141 / 141 / 201 bins with intg 10 / 10 / 10 / 20 on
    one ring (three sets of forward spectra, the largest group count 10, the longest look-back 21 periods): run as the
    full list, as subsets on an engine whose buffers are poisoned, and repeated over the same list -- a listed
    channel's result and power array are bit for bit the same in all of them.  Against the restatement as well."""
    sc = cc.SCEN["mixed"]
    W, pairs, wants = cc.scenario(gc, orc, synth, "mixed")
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    assert [(c.ncoh, c.nfreq, c.intg) for c in chans] == [(1, 71, 10), (5, 141, 10), (5, 141, 10), (10, 201, 20)]
    _load(engine, sc, W)
    engine.set_channels(chans)
    engine.acq_run(len(W))
    full = _check_results(engine, chans, wants, "mixed")
    assert all(r["flagacq"] for r in full) and [r["iters"] for r in full] == [1, 5, 5, 10]
    Pfull = [engine.acq_power(i).tobytes() for i in range(4)]
    _check_power(engine, orc, 3, chans[3], ochs[3], wants[3], (W, len(W)), "mixed")
    engine.acq_run(len(W))                                  # repeated over the same list
    assert engine.acq_fetch() == full
    assert [engine.acq_power(i).tobytes() for i in range(4)] == Pfull
    other = gc.Engine(0)
    try:
        other.debug_poison(0xA5)
        _load(other, sc, W)
        other.set_channels(chans)
        for sub in ([3], [1, 0], [2], [2, 3, 1]):
            other.acq_run(len(W), channels=sub)
            res = other.acq_fetch()
            for i in range(4):
                if i in sub:
                    assert res[i] == full[i], (sub, i)
                    assert other.acq_power(i).tobytes() == Pfull[i], (sub, i)
                else:
                    assert res[i]["flagacq"] == 0 and res[i]["iters"] == 0, (sub, i)
    finally:
        other.close()


# ---- 5. ring wrap and late positions -------------------------------------------------------------------------------
def test_group_span_across_the_ring_end(gc, orc, synth, engine):
    """A ring of (intg+3)*nsamp samples (rounded up to the ring's granule) that ends 7.5 periods into the search span:
    inside the one group of 10 and inside the second group of 5.  The stream goes in by several pushes; the
    restatement reads the same ring order."""
    sc = cc.SCEN["iq10"]
    W, pairs, ref = cc.scenario(gc, orc, synth, "iq10")
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    n = chans[0].nsamp
    ringlen = _granule(13 * n, 2)
    b0 = ringlen - (7 * n + n // 2)
    wrpos = b0 + len(W)
    stream = np.concatenate([ac.noise(b0, 2, 77), W])
    engine.ring_create(1, 2, ringlen)
    cc.push_wrapping(engine, 1, stream, wrpos, ringlen)
    assert engine.ring_wrpos(1) == wrpos
    engine.set_channels(chans)
    buf = cc.ring_order(stream, ringlen, wrpos)
    wants = ac.run_oracles([lambda o=o, c=c: cc.coh_acq(orc, o, buf, ringlen, wrpos, c.ncoh) for c, o in pairs])
    for w, r in zip(wants, ref):                            # the same samples: the same search
        assert w["b0"] == b0 and w["steps"] == r["steps"] and w["buffloc"] == r["buffloc"] + b0
    engine.acq_run(wrpos)
    res = _check_results(engine, chans, wants, "wrap")
    assert [(r["flagacq"], r["iters"]) for r in res] == [(1, 10), (1, 5), (1, 10), (0, 10)]
    for i in (0, 2):
        _check_power(engine, orc, i, chans[i], ochs[i], wants[i], (buf, ringlen), "wrap")


def test_search_past_2_32(gc, orc, synth, engine):
    """A write position past 2^32 samples, the groups' spans across it (ring_commit; the ring of
    tests/test_gpu_positions.py, whose length divides neither 2^31 nor 2^32)."""
    from test_gpu_positions import high_layout, high_ring
    W, pairs, ref = cc.scenario(gc, orc, synth, "iq10")
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    n, T = chans[0].nsamp, 1 << 32
    R, K = high_layout(T, 12 * n, 8, 7 * n, 8 * n)
    D = np.concatenate([ac.noise(R - len(W), 2, 78), W])
    wp = high_ring(engine, 1, 2, D, R, K)
    b0 = wp - len(W)
    assert b0 + 2 * n < T < b0 + 5 * n
    engine.set_channels(chans)
    wants = ac.run_oracles([lambda o=o, c=c: cc.coh_acq(orc, o, D, R, wp, c.ncoh) for c, o in pairs])
    for w, r in zip(wants, ref):
        assert w["steps"] == r["steps"] and w["buffloc"] == r["buffloc"] + b0
    engine.acq_run(wp)
    res = _check_results(engine, chans, wants, "2^32")
    assert all(r["buffloc"] >= T - 4 * n for r in res) and res[3]["buffloc"] == b0 + 10 * n > T
    _check_power(engine, orc, 2, chans[2], ochs[2], wants[2], (D, R), "2^32")


# ---- 6. / 7. real samples, the 65536-point path --------------------------------------------------------------------
def test_real_samples_at_an_if(gc, orc, synth, engine):
    """dtype 1, IF 4.092 MHz at 16.368 Msps (nsamp 16368), 9 bins, intg 4 with ncoh 2 and 4, the satellite in a bin
    below the IF centre.  The carrier tables walk 3 and 5 periods at ~8 LUT steps a sample without overflowing (the
    run would refuse)."""
    chans, res, wants = _scenario_on_engine(engine, gc, orc, synth, "real", power=(0, 1))
    assert [(c.ncoh, c.nsamp, c.nfreq) for c in chans] == [(2, 16368, 9), (4, 16368, 9)]
    assert [(r["flagacq"], r["iters"], r["freqi"]) for r in res] == [(1, 4, 3), (1, 4, 3)]
    assert res[0]["acqfreq"] == 4.092e6 - 250.0


def test_65536_point_path(gc, orc, synth, engine):
    """20 Msps, nsamp 20000, 9 bins, intg 4, ncoh 2: acq_fwd's four-residue transform and acq_corr64, second group."""
    chans, res, wants = _scenario_on_engine(engine, gc, orc, synth, "m20", power=(0,))
    assert chans[0].nsamp == 20000 and (res[0]["flagacq"], res[0]["iters"]) == (1, 4)


# ---- 8. data bit flip ----------------------------------------------------------------------------------------------
def test_bit_flip_span(gc, orc, synth, engine):
    """The weak satellite's span with its data bit flipped in the middle: not acquired, the restatement's peak ratio.
    And the 40 dB-Hz one, which both sides acquire two bins off."""
    chans, res, wants = _scenario_on_engine(engine, gc, orc, synth, "flip", power=(0,))
    assert not res[0]["flagacq"] and res[0]["peakr"] < 3.0 and res[0]["iters"] == 10
    print("flipped span: peakr device %.4f restatement %.4f" % (res[0]["peakr"], wants[0]["peakr"]))
    other = gc.Engine(0)
    try:
        chans, res, wants = _scenario_on_engine(other, gc, orc, synth, "flip40")
        assert res[0]["flagacq"] and res[0]["freqi"] == 3
    finally:
        other.close()


# ---- 9. hand-over --------------------------------------------------------------------------------------------------
def test_handover_and_schedule(gc, orc, synth, engine):
    """After a search with groups, trk_start_from_acq and loop_start_from_acq leave what acq_start_state defines for
    the restated result (carrfreq = acqfreq, codefreq = crate, zero remainders, buffloc) on the acquired channels and
    nothing on the other; and a two-step gnsscorr_rx_step run takes the channels from SEARCH to TRACK at the step the
    host's replay of the schedule says: the first whose write position reaches (intg+1)*nsamp."""
    sc = cc.SCEN["iq10"]
    W, pairs, wants = cc.scenario(gc, orc, synth, "iq10")
    chans = [c for c, _ in pairs]
    _load(engine, sc, W)
    engine.set_channels(chans)
    keep = [dict(carrfreq=300.0 * i, codefreq=c.crate + 1.0, remcode=0.5, remcarr=1.0, buffloc=4321 * (i + 1))
            for i, c in enumerate(chans)]
    want_state = [dict(carrfreq=w["acqfreq"], codefreq=c.crate, remcode=0.0, remcarr=0.0, buffloc=w["buffloc"])
                  if w["flagacq"] else k for c, w, k in zip(chans, wants, keep)]
    engine.trk_set_state(keep)
    engine.loop_set([engine.loop_state(i, 1.0 + i, flagsync=1, synci=3, cnt=100 + i) for i in range(4)])
    engine.acq_run(len(W))
    _check_results(engine, chans, wants, "handover")
    engine.trk_start_from_acq()
    assert engine.trk_get_state() == want_state
    engine.trk_set_state(keep)
    engine.loop_start_from_acq()
    assert engine.trk_get_state() == want_state
    for i, (ls, w) in enumerate(zip(engine.loop_get(), wants)):
        if w["flagacq"]:
            assert (ls.acqfreq, ls.cnt, ls.flagsync, ls.prn) == (w["acqfreq"], 0, 0, chans[i].prn), i
        else:
            assert (ls.acqfreq, ls.cnt, ls.flagsync) == (1.0 + i, 100 + i, 1), i

    # the schedule: host replay (gnsscorr_rx_step's rules: due at wp >= next_try = (intg+1)*nsamp, TRACK when acquired)
    first = 7 * chans[0].nsamp
    steps = [first, len(W)]
    replay = []
    state = [gc.CH_SEARCH] * 4
    for wp in steps:
        for i, (c, w) in enumerate(zip(chans, wants)):
            if state[i] == gc.CH_SEARCH and wp >= (c.intg + 1) * c.nsamp and w["flagacq"]:
                state[i] = gc.CH_TRACK
        replay.append(list(state))
    assert replay == [[gc.CH_SEARCH] * 4, [gc.CH_TRACK] * 3 + [gc.CH_SEARCH]]
    rx = gc.Engine(0)
    try:
        ringlen = _granule(len(W), 2)
        rx.ring_create(1, 2, ringlen)
        rx.set_channels(chans)
        rx.loop_set([rx.loop_state(i, 0.0) for i in range(4)])
        rx.rx_start()
        at = 0
        for wp, want in zip(steps, replay):
            rx.ring_push_raw(1, W[at:wp], wp - at)
            at = wp
            rx.rx_step(5)
            st = rx.rx_status()
            assert [s["state"] for s in st] == want, wp
        for s, w, c, ws in zip(st, wants, chans, want_state):
            assert s["attempts"] == 1 and s["acq_wrpos"] == len(W)
            ac.check_result(s["acq"], w, ("rx", c.prn))
        _, ndone = rx.trk_fetch_log()
        assert np.all(ndone[:3] >= 1) and ndone[3] == 0
        ls = rx.loop_get()
        assert [l.acqfreq for l in ls[:3]] == [w["acqfreq"] for w in wants[:3]]
    finally:
        rx.close()


# ---- 10. refusals --------------------------------------------------------------------------------------------------
def test_refusals_leave_the_setting(gc, orc, synth, engine):
    """Every refusal of gnsscorr_acq_set_coherent leaves the previous setting in place and working; set_channels
    resets every channel to 1; acq_power on a channel the last run did not list is still refused."""
    sc = cc.SCEN["iq10"]
    W, pairs, wants = cc.scenario(gc, orc, synth, "iq10")
    chans = [c for c, _ in pairs]
    plain = [gc.Channel(c.prn, dtype=2, f_sf=c.f_sf, f_if=0.0, hband=h, step=s, intg=i)
             for c, (_, h, s, i, _) in zip(chans, sc["chans"])]
    _load(engine, sc, W)
    with pytest.raises(gc.GnsscorrError):
        engine.acq_set_coherent([1])                        # no channels yet
    engine.set_channels(plain)
    assert engine.acq_get_coherent() == [1, 1, 1, 1]
    setting = [10, 5, 5, 5]
    engine.acq_set_coherent(setting)
    engine.acq_run(len(W))
    before = engine.acq_fetch()
    bad = [([0], 0), ([-1], 1), ([21], 0), ([3], 1), ([20], 2), ([4], 3),        # < 1, > MAXCOH, not a divisor of 10
           ([5, 5, 5, 5, 5], 0), ([5], 4), ([5], -1), ([5, 5], 3), ([], 0),    # a range outside the table
           ([2, 2, 3, 2], 0)]                                                   # one bad entry: nothing is touched
    for ncoh, ch0 in bad:
        with pytest.raises(gc.GnsscorrError):
            engine.acq_set_coherent(ncoh, ch0=ch0)
        assert engine.acq_get_coherent() == setting, (ncoh, ch0)
    assert engine.acq_fetch() == before                     # (a refusal does not drop the last search either)
    engine.acq_run(len(W))
    assert engine.acq_fetch() == before
    _check_results(engine, chans, wants, "after refusals")
    engine.acq_run(len(W), channels=[0, 2])
    with pytest.raises(gc.GnsscorrError):
        engine.acq_power(1)
    assert engine.acq_power(2).shape == (9, 4092)
    engine.acq_set_coherent([1], ch0=1)                     # a change drops the last search: fetch refuses until the next
    with pytest.raises(gc.GnsscorrError):
        engine.acq_fetch()
    assert engine.acq_get_coherent() == [10, 1, 5, 5]
    engine.set_channels(plain)
    assert engine.acq_get_coherent() == [1, 1, 1, 1]
