"""Bit-edge hypotheses for coherent groups (gnsscorr_acq_set_bitedge) on the device against the restatement of their
semantics (tests/acq_edge_cases.py; parity tests proper, -m gpu).  tests/test_acq_edge_host.py shows on the host that
every scenario here is decided with room.

Bars, those of tests/test_gpu_acq_coherent.py: flagacq, iters, buffloc, acqcodei, freqi and acqfreq identical to the
restatement's; peakr and cn0 to 1e-4; acq_fetch_edge identical; the device's cn0 within 1e-9 of checkacquisition()'s
formula over its own power array and ncoh*ctime; acq_power element-wise, |P_gpu - P_td| <= acq_cases.POWER_TOL x (the
Doppler row's mean outside the exclusion window), P_td the fp64 time-domain sum of the hypotheses the restatement chose
(acq_edge_cases.edge_power_td).  Rows whose two best hypotheses lie within MARGIN of each other in some group may choose
differently in fp32 and are left out of the element-wise check: at most 5 % of a channel's rows, never the deciding one
(asserted on the host).

Measured on the MI355X (every check prints its ratio and the largest so far): the largest was 8.3e-5, in
test_step_two (45 dB-Hz, one group of 10, the peak 312 times the row's mean, lag 3210) and 8.2e-5 in
test_mixed_list_subsets_and_repeat (42 dB-Hz, ncoh 10, estep 5); 1.7e-5 to 4.8e-5 for the other acquired channels,
below 1e-5 for the absent PRNs.  The checked satellites sit at lags where the search without hypotheses meets the bar as
well (acq_edge_cases.SCEN says why).  The file runs in about 6 s."""
import ctypes as C

import numpy as np
import pytest

import acq_cases as ac
import acq_coh_cases as cc
import acq_edge_cases as ec

pytestmark = pytest.mark.gpu

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
    edge = engine.acq_fetch_edge()
    for i, (c, r, w) in enumerate(zip(chans, res, wants)):
        ac.check_result(r, w, (where, i, c.prn, c.ncoh, c.estep))
        assert edge[i] == w["edge"], (where, i, c.prn, edge[i], w["edge"])
    return res, edge


def _check_power(engine, orc, i, c, o, want, ring, where="", seed=0):
    """acq_power of channel i: shape, the device's cn0 over its own array, and the element-wise bar at the lags of
    acq_cases.check_lags in every row that did not tie on its hypothesis."""
    buf, ringlen = ring
    P = engine.acq_power(i)
    assert P.shape == want["P"].shape
    r = engine.acq_fetch()[i]
    cn0 = ac._cn0_restated(P, r["acqcodei"], r["freqi"], c.nsampchip, c.ncoh * c.ctime)
    assert abs(r["cn0"] - cn0) <= 1e-9 * abs(cn0), (where, i, r["cn0"], cn0)
    keep = ~ec.tied_rows(want)
    assert keep[want["freqi"]] and (~keep).mean() <= ec.TIE_CAP
    lags = ac.check_lags(o, want["acqcodei"], np.random.default_rng(seed + i))
    td = ec.edge_power_td(orc, o, buf, ringlen, want["b0"], want["groups"], c.ncoh, want["hsel"], lags)
    ratio = ac.power_ratio(P[keep], td[keep], lags, want["P"][keep], want["acqcodei"], c.nsampchip)
    _ratios.append(ratio)
    print(f"power {where} ch {i} prn {c.prn} ncoh {c.ncoh} estep {c.estep} groups {want['groups']} rows left out "
          f"{int((~keep).sum())}: max |dP|/meanP {ratio:.3g} (largest so far {max(_ratios):.3g})")
    assert ratio <= ac.POWER_TOL, (where, i, ratio)
    return P


def _scenario_on_engine(engine, gc, orc, synth, name, power=()):
    """The scenario as tests/acq_edge_cases.py states it: ring = its span, the search ends at the span's last sample."""
    sc = ec.SCEN[name]
    W, pairs, wants = ec.scenario(gc, orc, synth, name)
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    _load(engine, sc, W)
    engine.set_channels(chans)
    assert engine.acq_get_coherent() == [c.ncoh for c in chans]
    assert engine.acq_get_bitedge() == [c.estep for c in chans]
    engine.acq_run(len(W))
    res, edge = _check_results(engine, chans, wants, name)
    for i in power:
        _check_power(engine, orc, i, chans[i], ochs[i], wants[i], (W, len(W)), name)
    return chans, res, edge, wants


# ---- 1. the scenarios against the restatement ----------------------------------------------------------------------
def test_edges_at_one_nine_none_and_mid_period(gc, orc, synth, engine):
    """One group of 10 with every hypothesis, 40 to 42 dB-Hz: edges at 1 and 9, no edge (edge 0), a flip 0.72 into
    period 4 (a boundary beside it: 4), an absent PRN (not acquired: -1)."""
    chans, res, edge, _ = _scenario_on_engine(engine, gc, orc, synth, "edges40", power=(0, 1, 2, 3, 4))
    assert edge == [1, 9, 0, 4, -1] and [r["flagacq"] for r in res] == [1, 1, 1, 1, 0]


def test_groups_of_five_choose_per_group(gc, orc, synth, engine):
    """intg 10 in groups of 5, the bit edge at span period 3: the strong satellite passes at group 1 with edge 3; the
    36.5 dB-Hz one only at group 2, its power the sum of the rows of h = 3 (group 1) and h = 0 (group 2), edge 0."""
    chans, res, edge, wants = _scenario_on_engine(engine, gc, orc, synth, "groups5", power=(0, 1, 2))
    assert [(r["flagacq"], r["iters"]) for r in res] == [(1, 5), (1, 10), (0, 10)] and edge == [3, 0, -1]
    assert [int(h[wants[1]["freqi"]]) for h in wants[1]["hsel"]] == [3, 0]


def test_step_two(gc, orc, synth, engine):
    """estep 2 (hypotheses 0, 2, 4, 6, 8): an edge on a hypothesis and one between two."""
    _, res, edge, _ = _scenario_on_engine(engine, gc, orc, synth, "step2", power=(0, 1))
    assert edge == [4, 6] and all(r["flagacq"] for r in res)


def test_real_samples_at_an_if(gc, orc, synth, engine):
    """dtype 1, IF 4.092 MHz at 16.368 Msps: nsamp 16368, every lag of the 32768-point path in use; one group of 4."""
    chans, res, edge, _ = _scenario_on_engine(engine, gc, orc, synth, "real", power=(0,))
    assert chans[0].nsamp == 16368 and edge == [2] and (res[0]["flagacq"], res[0]["iters"]) == (1, 4)


# ---- 2. the pilot, end to end --------------------------------------------------------------------------------------
def test_weak_satellite_with_a_bit_edge_and_the_schedule(gc, orc, synth, engine):
    """The 36 dB-Hz satellite whose bit flips on its fifth period boundary, three channels on its PRN: without
    hypotheses not acquired, with estep 1 acquired at its lag and bin with edge 5, with estep 2 not acquired.  Then the
    same through gnsscorr_rx_start / gnsscorr_rx_step: the estep 1 channel reaches TRACK with the restatement's result,
    the others stay in SEARCH."""
    chans, res, edge, wants = _scenario_on_engine(engine, gc, orc, synth, "edge36", power=(1,))
    assert [(c.ncoh, c.estep, c.nfreq) for c in chans] == [(10, 0, 201), (10, 1, 201), (10, 2, 201)]
    assert [r["flagacq"] for r in res] == [0, 1, 0] and edge == [-1, 5, -1]
    assert abs(res[1]["acqcodei"] - 1234) <= 1 and res[1]["freqi"] == 120 and res[1]["iters"] == 10
    print("bit edge at 5: estep 0 peakr %.3f; estep 1 peakr %.3f cn0 %.2f; estep 2 peakr %.3f"
          % (res[0]["peakr"], res[1]["peakr"], res[1]["cn0"], res[2]["peakr"]))
    W = ec.scenario(gc, orc, synth, "edge36")[0]
    rx = gc.Engine(0)
    try:
        rx.ring_create(1, 2, _granule(len(W), 2))
        rx.set_channels(chans)
        rx.loop_set([rx.loop_state(i, 0.0) for i in range(3)])
        rx.rx_start()
        at = 0
        for wp, want in ((7 * chans[0].nsamp, [gc.CH_SEARCH] * 3), (len(W), [gc.CH_SEARCH, gc.CH_TRACK, gc.CH_SEARCH])):
            rx.ring_push_raw(1, W[at:wp], wp - at)
            at = wp
            rx.rx_step(5)
            st = rx.rx_status()
            assert [s["state"] for s in st] == want, wp
        for s, w, c in zip(st, wants, chans):
            assert s["attempts"] == 1 and s["acq_wrpos"] == len(W)
            ac.check_result(s["acq"], w, ("rx", c.estep))
        assert rx.acq_fetch_edge() == [-1, 5, -1]
        _, ndone = rx.trk_fetch_log()
        assert ndone[1] >= 1 and ndone[0] == 0 and ndone[2] == 0
        assert rx.loop_get()[1].acqfreq == wants[1]["acqfreq"]
    finally:
        rx.close()


# ---- 3. estep 0: nothing changes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["groups5", "real"])
def test_all_zero_is_bitwise_the_engine_that_never_called_it(gc, synth, engine, name):
    """After acq_set_bitedge with all zeros, results and power arrays are bit for bit those of an engine that never
    called it, and every edge is -1."""
    sc = ec.SCEN[name]
    W = cc.make_span(gc, synth, sc)
    chans = [gc.Channel(p, dtype=sc["dtype"], f_sf=sc["f_sf"], f_if=sc["f_if"], hband=h, step=s, intg=i, ncoh=k)
             for p, h, s, i, k, _ in sc["chans"]]
    other = gc.Engine(0)
    try:
        out = []
        for e, call in ((engine, False), (other, True)):
            _load(e, sc, W)
            e.set_channels(chans)
            if call:
                e.acq_set_bitedge([0] * len(chans))
            assert e.acq_get_bitedge() == [0] * len(chans)
            e.acq_run(len(W))
            assert e.acq_fetch_edge() == [-1] * len(chans)
            out.append((e.acq_fetch(), [e.acq_power(i).tobytes() for i in range(len(chans))]))
        assert out[0][0] == out[1][0]
        assert out[0][1] == out[1][1]
        assert all(r["iters"] > 0 for r in out[0][0])
    finally:
        other.close()


# ---- 4. mixed grids: lists, subsets, repeats -----------------------------------------------------------------------
def test_mixed_list_subsets_and_repeat(gc, orc, synth, engine):
    """One ring with an ncoh 1 channel (10 slots of forward spectra), an ncoh 5 channel without hypotheses (2), one
    with estep 1 (2 x 5) and an ncoh 10 / intg 20 channel with estep 5 (2 x 2): against the restatement; repeated; as
    subsets on a poisoned engine; and the two channels without hypotheses bit for bit what an engine that holds only
    them computes."""
    sc = ec.SCEN["mixed"]
    W, pairs, wants = ec.scenario(gc, orc, synth, "mixed")
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    assert [(c.ncoh, c.estep, c.nfreq, c.intg) for c in chans] == [(1, 0, 21, 10), (5, 0, 41, 10), (5, 1, 41, 10),
                                                                   (10, 5, 61, 20)]
    _load(engine, sc, W)
    engine.set_channels(chans)
    engine.acq_run(len(W))
    full, edge = _check_results(engine, chans, wants, "mixed")
    assert all(r["flagacq"] for r in full) and [r["iters"] for r in full] == [1, 5, 5, 10] and edge == [-1, -1, 2, 5]
    Pfull = [engine.acq_power(i).tobytes() for i in range(4)]
    for i in (2, 3):
        _check_power(engine, orc, i, chans[i], ochs[i], wants[i], (W, len(W)), "mixed")
    engine.acq_run(len(W))                                  # repeated over the same list
    assert engine.acq_fetch() == full and engine.acq_fetch_edge() == edge
    assert [engine.acq_power(i).tobytes() for i in range(4)] == Pfull
    other = gc.Engine(0)
    try:
        other.debug_poison(0xA5)
        _load(other, sc, W)
        other.set_channels(chans)
        for sub in ([3], [2, 0], [1], [1, 3, 2], [0, 1]):
            other.acq_run(len(W), channels=sub)
            res, ed = other.acq_fetch(), other.acq_fetch_edge()
            for i in range(4):
                if i in sub:
                    assert res[i] == full[i] and ed[i] == edge[i], (sub, i)
                    assert other.acq_power(i).tobytes() == Pfull[i], (sub, i)
                else:
                    assert res[i]["flagacq"] == 0 and res[i]["iters"] == 0 and ed[i] == -1, (sub, i)
        # without the channels that have hypotheses
        other.set_channels(chans[:2])
        assert other.acq_get_bitedge() == [0, 0]
        other.acq_run(len(W))
        assert other.acq_fetch() == full[:2] and other.acq_fetch_edge() == [-1, -1]
        assert [other.acq_power(i).tobytes() for i in range(2)] == Pfull[:2]
    finally:
        other.close()


# ---- 5. refusals and resets ----------------------------------------------------------------------------------------
def test_refusals_and_resets(gc, orc, synth, engine):
    """Every refusal of gnsscorr_acq_set_bitedge leaves the setting and the last search in place; acq_set_coherent
    resets the channels it names, set_channels all; fetch_edge before a search is GNSSCORR_ESTATE."""
    L = gc.lib()
    sc = ec.SCEN["groups5"]
    W, pairs, wants = ec.scenario(gc, orc, synth, "groups5")
    chans = [c for c, _ in pairs]
    plain = [gc.Channel(c.prn, dtype=2, f_sf=c.f_sf, f_if=0.0, hband=h, step=s, intg=i)
             for c, (_, h, s, i, _, _) in zip(chans, sc["chans"])]
    _load(engine, sc, W)
    buf = (C.c_int * 4)()
    with pytest.raises(gc.GnsscorrError):
        engine.acq_set_bitedge([0])                         # no channels yet
    engine.set_channels(plain)
    assert L.gnsscorr_acq_fetch_edge(engine.h, buf) == -3   # GNSSCORR_ESTATE: no search yet
    assert engine.acq_get_bitedge() == [0, 0, 0] and engine.acq_get_coherent() == [1, 1, 1]
    with pytest.raises(gc.GnsscorrError) as e:
        engine.acq_set_bitedge([0, 1, 0])                   # estep >= 1 on a channel with ncoh 1
    assert "channel 1" in str(e.value)
    engine.acq_set_coherent([5, 5, 10])
    setting = [1, 4, 9]
    engine.acq_set_bitedge(setting)
    assert L.gnsscorr_acq_fetch_edge(engine.h, buf) == -3   # the change dropped nothing to fetch either
    engine.acq_run(len(W))
    before, edge = engine.acq_fetch(), engine.acq_fetch_edge()
    bad = [([-1], 0), ([5], 0), ([6], 1), ([10], 2), ([1, 1, 1, 1], 0), ([1], 3), ([1], -1), ([1, 1], 2), ([], 0),
           ([2, 2, 10], 0), ([0, -2], 1)]                   # < 0, >= ncoh, a range outside the table, one bad entry
    for estep, ch0 in bad:
        with pytest.raises(gc.GnsscorrError):
            engine.acq_set_bitedge(estep, ch0=ch0)
        assert engine.acq_get_bitedge() == setting and engine.acq_get_coherent() == [5, 5, 10], (estep, ch0)
    assert engine.acq_fetch() == before and engine.acq_fetch_edge() == edge     # (a refusal drops no search)
    engine.acq_run(len(W))
    assert engine.acq_fetch() == before and engine.acq_fetch_edge() == edge
    engine.acq_set_coherent([5], ch0=1)                     # resets the channel it names, and drops the search
    assert engine.acq_get_bitedge() == [1, 0, 9]
    assert L.gnsscorr_acq_fetch_edge(engine.h, buf) == -3
    engine.acq_set_bitedge([0], ch0=2)
    assert engine.acq_get_bitedge() == [1, 0, 0]
    engine.set_channels(plain)
    assert engine.acq_get_bitedge() == [0, 0, 0]
    # the scenario still runs on this engine afterwards
    engine.set_channels(chans)
    assert engine.acq_get_bitedge() == [1, 1, 1]
    engine.acq_run(len(W))
    _check_results(engine, chans, wants, "after refusals")


def test_the_65536_point_path_is_refused(gc, synth, engine):
    """The transform length is the context's: with a 20 Msps channel (nsamp 20000) beside a 4.092 Msps one on another
    ring, gnsscorr_acq_set_bitedge refuses, whichever channel it names, and the coherent search still runs."""
    sc = cc.SCEN["m20"]
    W = cc.make_span(gc, synth, sc)
    _load(engine, sc, W, ftype=1)
    engine.ring_create(2, 2, 4092 * 16)
    big = gc.Channel(20, dtype=2, f_sf=20e6, f_if=0.0, hband=1000, step=250, intg=4, ncoh=2)
    small = gc.Channel(9, dtype=2, ftype=2, f_sf=4.092e6, f_if=0.0, hband=200, step=50, intg=10, ncoh=10)
    engine.set_channels([big, small])
    for estep, ch0 in (([1], 1), ([1], 0), ([1, 1], 0)):
        with pytest.raises(gc.GnsscorrError) as e:
            engine.acq_set_bitedge(estep, ch0=ch0)
        assert "nsamp 20000" in str(e.value)
    assert engine.acq_get_bitedge() == [0, 0]
    with pytest.raises(gc.GnsscorrError):
        engine.set_channels([big, gc.Channel(9, dtype=2, ftype=2, f_sf=4.092e6, f_if=0.0, hband=200, step=50, intg=10,
                                             ncoh=10, estep=1)])
    engine.set_channels([big])
    engine.acq_run(len(W))
    assert engine.acq_fetch()[0]["flagacq"] == 1 and engine.acq_fetch_edge() == [-1]
