"""Carrier frequency refinement of acquired channels (gnsscorr_acq_set_refine) on the device against
the restatement of its semantics (tests/acq_fine_cases.py; parity tests proper, -m gpu).  tests/test_acq_fine_host.py
shows on the host that every scenario here decides q* with a relative gap above 1e-9 and that the restated search finds
its satellites where the device does.

Bars: the prompt sums bit for bit, q and nref equal, finefreq to 1e-9 Hz and quality to 1e-9 relative, the restatement
being run on the search result the device itself fetched (which is also held against the restated search); whatever the
refinement does not own -- results, edges, power arrays, the hand-over of a channel with nref = 0 -- bit for bit what
it is without it."""
import ctypes as C

import numpy as np
import pytest

import acq_cases as ac
import acq_edge_cases as ec
import acq_fine_cases as fc

pytestmark = pytest.mark.gpu

F4 = 4.092e6


def _load(engine, sc, W, ftype=1):
    ringlen = ec.granule(len(W), sc["dtype"])
    engine.ring_create(ftype, sc["dtype"], ringlen)
    engine.ring_push_raw(ftype, W, len(W))
    assert engine.ring_wrpos(ftype) == len(W)
    return ringlen


def _check_fine(engine, orc, pairs, buf, ringlen, nref, where="", listed=None):
    """fetch_fine of the last search against the restatement on the device's own search results.  nref: per channel.
    Returns (results, fine, prompts)."""
    res = engine.acq_fetch()
    fine, P = engine.acq_fetch_fine(prompts=True)
    assert [f == g for f, g in zip(fine, engine.acq_fetch_fine())] == [True] * len(pairs)
    want = fc.fine_all(orc, pairs, buf, ringlen, res, nref)
    for i, (f, w) in enumerate(zip(fine, want)):
        if listed is not None and i not in listed:
            continue
        at = (where, i, pairs[i][0].prn)
        assert np.array_equal(P[i], w["prompt"]), at
        assert (f["q"], f["nref"]) == (w["q"], w["nref"]), (at, f, w["q"], w["nref"])
        assert abs(f["finefreq"] - w["finefreq"]) <= 1e-9, (at, f["finefreq"], w["finefreq"])
        assert abs(f["quality"] - w["quality"]) <= 1e-9 * w["quality"], (at, f["quality"], w["quality"])
        if w["nref"]:
            assert w["gap"] > fc.GAP and 0.0 < f["quality"] <= 1.0 + 1e-12, (at, w["gap"], f["quality"])
    return res, fine, P


def _scenario_on_engine(engine, gc, orc, synth, name, nref):
    sc = fc.SCEN[name]
    W, pairs, wants = fc.scenario(gc, orc, synth, name)
    chans = [c for c, _ in pairs]
    _load(engine, sc, W)
    engine.set_channels(chans)
    assert engine.acq_get_refine() == [0] * len(chans)
    engine.acq_set_refine([nref] * len(chans))
    assert engine.acq_get_refine() == [nref] * len(chans)
    engine.acq_run(len(W))
    res, fine, P = _check_fine(engine, orc, pairs, W, len(W), nref, (name, nref))
    for c, r, w in zip(chans, res, wants):
        ac.check_result(r, w, (name, c.prn))
    return sc, W, pairs, res, fine, P


# ---- 1. parity with the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", [(n, w) for n in sorted(fc.SCEN) for w in (0, 1)])
def test_parity_with_the_restatement(gc, orc, synth, engine, name, which):
    """Every scenario with nref 2 and nref = intg: IQ and real samples at 4.092 Msps, 2.048 Msps, a group of ten with
    bit-edge hypotheses, and periods of 26000 samples (the 65536-point search, the largest prompt sums).  The refined
    frequency is nearer the satellite's than the bin centre for nref = intg."""
    nref = fc.nrefs(fc.SCEN[name])[which]
    sc, W, pairs, res, fine, P = _scenario_on_engine(engine, gc, orc, synth, name, nref)
    for (c, _), r, f in zip(pairs, res, fine):
        ft = fc.f_true(sc, c.prn)
        if ft is None:
            assert not r["flagacq"] and (f["finefreq"], f["quality"], f["q"], f["nref"]) == (r["acqfreq"], 0.0, 0, 0)
            continue
        assert r["flagacq"] and f["nref"] == nref
        print(f"{name} prn {c.prn} nref {nref}: coarse error {r['acqfreq'] - ft:+.1f} Hz, fine {f['finefreq'] - ft:+.2f} Hz, "
              f"quality {f['quality']:.3f}")
        assert abs(f["finefreq"] - ft) <= 1.0 / (4.0 * nref * c.ctime)
        if which:
            assert abs(f["finefreq"] - ft) < abs(r["acqfreq"] - ft)


@pytest.mark.parametrize("name,point", [("iq4", p) for p in sorted(ac.wrap_points(fc.N4, 10))] + [("real4", "iteration_start")])
def test_ring_wraps_inside_the_span(gc, orc, synth, engine, name, point):
    """The ring, exactly one search span long, ends at each of the span's wrap points: inside the refine spans' first
    period, on a period boundary, in the last window and one sample before the write position.  The stream goes in by
    several pushes; the restatement reads the same ring order."""
    sc = fc.SCEN[name]
    W, pairs, wants = fc.scenario(gc, orc, synth, name)
    chans = [c for c, _ in pairs]
    n, intg, dtype = chans[0].nsamp, chans[0].intg, sc["dtype"]
    ringlen = ec.granule(len(W), dtype)
    b0 = ringlen - ac.wrap_points(n, intg)[point]
    stream, ringlen, wrpos = ec.placed(W, dtype, ringlen, b0)
    engine.ring_create(1, dtype, ringlen)
    fc.push_wrapping(engine, 1, stream, wrpos, ringlen)
    assert engine.ring_wrpos(1) == wrpos and b0 < ringlen < wrpos
    engine.set_channels(chans)
    engine.acq_set_refine([intg] * len(chans))
    engine.acq_run(wrpos)
    buf = fc.ring_order(stream, ringlen, wrpos)
    res, fine, P = _check_fine(engine, orc, pairs, buf, ringlen, intg, (name, point))
    ref = fc.fine_all(orc, pairs, W, len(W), wants, intg)           # the same samples: the same refinement
    inside = 0
    for r, w, f, g in zip(res, wants, fine, ref):
        assert r["buffloc"] == w["buffloc"] + b0 and (f["q"], f["nref"]) == (g["q"], g["nref"])
        inside += bool(r["flagacq"]) and r["buffloc"] < ringlen < r["buffloc"] + intg * n
    assert inside or point in ("last_window", "before_wrpos")


def test_write_positions_past_2_32(gc, orc, synth, engine):
    """A write position past 2^32 samples, the refine spans across it (ring_commit; the ring of
    tests/test_gpu_positions.py, whose length divides neither 2^31 nor 2^32)."""
    from test_gpu_positions import high_layout, high_ring
    W, pairs, wants = fc.scenario(gc, orc, synth, "iq4")
    chans = [c for c, _ in pairs]
    n, T = chans[0].nsamp, 1 << 32
    R, K = high_layout(T, 12 * n, 8, 7 * n, 8 * n)
    D = np.concatenate([ac.noise(R - len(W), 2, 78), W])
    wp = high_ring(engine, 1, 2, D, R, K)
    b0 = wp - len(W)
    assert b0 + 2 * n < T < b0 + 5 * n
    engine.set_channels(chans)
    engine.acq_set_refine([10] * len(chans))
    engine.acq_run(wp)
    res, fine, P = _check_fine(engine, orc, pairs, D, R, 10, "2^32")
    ref = fc.fine_all(orc, pairs, W, len(W), wants, 10)
    for r, w, f, g in zip(res, wants, fine, ref):
        assert r["buffloc"] == w["buffloc"] + b0 and (f["q"], f["nref"]) == (g["q"], g["nref"])
        assert not r["flagacq"] or r["buffloc"] < T < r["buffloc"] + 10 * n


# ---- 2. nothing else moves -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["iq4", "coh", "m26"])
def test_nothing_else_moves(gc, orc, synth, engine, name):
    """A context with nref > 0 on some channels beside one that never called set_refine, on the same input: results,
    edges and power arrays bit for bit.  With nref = 0 on all channels fetch_fine gives rule 8 in both."""
    sc = fc.SCEN[name]
    W, pairs, _ = fc.scenario(gc, orc, synth, name)
    chans = [c for c, _ in pairs]
    nref = [(sc["chans"][0][3], 0, 2)[i % 3] for i in range(len(chans))]
    other = gc.Engine(0)
    try:
        out = []
        for e, call in ((engine, True), (other, False)):
            _load(e, sc, W)
            e.set_channels(chans)
            if call:
                e.acq_set_refine(nref)
            e.acq_run(len(W))
            out.append((e.acq_fetch(), e.acq_fetch_edge(), [e.acq_power(i).tobytes() for i in range(len(chans))]))
        assert out[0] == out[1]
        _check_fine(engine, orc, pairs, W, len(W), nref, name)
        engine.acq_set_refine([0] * len(chans))
        assert engine.acq_fetch() == out[0][0]                  # set_refine keeps the last search
        engine.acq_run(len(W))
        assert (engine.acq_fetch(), engine.acq_fetch_edge()) == out[0][:2]
        for e in (engine, other):
            fine, P = e.acq_fetch_fine(prompts=True)
            assert fine == [dict(finefreq=r["acqfreq"], quality=0.0, q=0, nref=0) for r in out[0][0]] and not P.any()
    finally:
        other.close()


# ---- 3. rule 8 -------------------------------------------------------------------------------------------------------
def test_rule_8_in_one_search(gc, orc, synth, engine):
    """One search with an absent PRN (nref 10), a channel with nref = 0 and a channel outside the list."""
    sc = fc.SCEN["iq4"]
    W, pairs, _ = fc.scenario(gc, orc, synth, "iq4")
    chans = [c for c, _ in pairs]
    assert fc.f_true(sc, chans[4].prn) is None
    nref, listed = [10, 0, 10, 10, 10], [0, 1, 2, 4]
    _load(engine, sc, W)
    engine.set_channels(chans)
    engine.acq_set_refine(nref)
    engine.acq_run(len(W), channels=listed)
    res, fine, P = _check_fine(engine, orc, pairs, W, len(W), nref, "rule 8", listed=listed)
    assert [r["flagacq"] for r in res] == [1, 1, 1, 0, 0]
    assert [f["nref"] for f in fine] == [10, 0, 10, 0, 0] and P[0].any() and P[2].any()
    for i in (1, 3, 4):
        assert fine[i] == dict(finefreq=res[i]["acqfreq"], quality=0.0, q=0, nref=0) and not P[i].any(), i
    assert fine[3]["finefreq"] == 0.0 and res[1]["acqfreq"] != 0.0 and res[4]["acqfreq"] != 0.0


# ---- 4. lists --------------------------------------------------------------------------------------------------------
def test_subset_equals_full_run(gc, orc, synth, engine):
    """A channel's fine result and prompts from acq_run_subset, on an engine whose buffers are poisoned, are bit for
    bit those of the full run; so is a repeat of the full run."""
    sc = fc.SCEN["iq4"]
    W, pairs, _ = fc.scenario(gc, orc, synth, "iq4")
    chans = [c for c, _ in pairs]
    nref = [10, 2, 0, 7, 10]
    _load(engine, sc, W)
    engine.set_channels(chans)
    engine.acq_set_refine(nref)
    engine.acq_run(len(W))
    res, fine, P = _check_fine(engine, orc, pairs, W, len(W), nref, "full")
    engine.acq_run(len(W))
    again = engine.acq_fetch_fine(prompts=True)
    assert again[0] == fine and again[1].tobytes() == P.tobytes()
    other = gc.Engine(0)
    try:
        other.debug_poison(0xA5)
        _load(other, sc, W)
        other.set_channels(chans)
        other.acq_set_refine(nref)
        for sub in ([3], [1, 0], [2], [4, 3, 1], [2, 4]):
            other.acq_run(len(W), channels=sub)
            f2, P2 = other.acq_fetch_fine(prompts=True)
            for i in range(len(chans)):
                if i in sub:
                    assert f2[i] == fine[i] and P2[i].tobytes() == P[i].tobytes(), (sub, i)
                else:
                    assert f2[i] == dict(finefreq=0.0, quality=0.0, q=0, nref=0) and not P2[i].any(), (sub, i)
    finally:
        other.close()


# ---- 5. hand-over ----------------------------------------------------------------------------------------------------
def test_handover_starts_from_the_refined_frequency(gc, orc, synth, engine):
    """trk_start_from_acq gives carrfreq = finefreq; after loop_start_from_acq tracking and loop state equal the host
    path acq_fetch -> loop_state -> loop_set with acqfreq replaced by the restatement's finefreq, bit for bit, and so
    are 200 closed-loop periods from there -- against that second engine and against the oracle's loop from the same
    state.  The channel with nref = 0 in the same context is handed over at its bin centre, the absent one not at
    all."""
    from test_gpu_loop import _check_against_oracle
    HO_PRNS, HO_DOP = fc.HO_PRNS, fc.HO_DOP
    sig = fc.handover_signal(gc, synth)
    nsig, n, wrpos = sig.shape[0], fc.N4, fc.HO_WRPOS
    mk = lambda: [c for c, _ in fc.handover_pairs(gc, orc)]  # noqa: E731
    pairs = fc.handover_pairs(gc, orc)
    keep = [dict(carrfreq=900.0 + i, codefreq=1.023e6 + 0.25 * i, remcode=0.125 * (i + 1), remcarr=0.5 + i,
                 buffloc=3000 + 17 * i) for i in range(3)]

    def prepare(e, nref):
        e.ring_create(1, 2, nsig)
        e.ring_push_raw(1, sig, nsig)
        e.set_channels(mk())
        if nref:
            e.acq_set_refine(nref)
        e.trk_set_state(keep)
        e.loop_set([e.loop_state(i, 800.0 + i, flagsync=1, synci=3 + i, cnt=4000 + i) for i in range(3)])
        e.acq_run(wrpos)

    host = gc.Engine(0)
    try:
        prepare(engine, [10, 0, 10])
        prepare(host, None)
        res, fine, _ = _check_fine(engine, orc, pairs, sig, nsig, [10, 0, 10], "handover")
        assert host.acq_fetch() == res and [r["flagacq"] for r in res] == [1, 1, 0]
        want = fc.fine_all(orc, pairs, sig, nsig, res, [10, 0, 10])
        freq = [want[0]["finefreq"], res[1]["acqfreq"]]
        assert fine[0]["finefreq"] == freq[0] != res[0]["acqfreq"] and fine[1]["finefreq"] == freq[1]
        assert abs(freq[0] - HO_DOP[0]) < 25.0 < abs(res[0]["acqfreq"] - HO_DOP[0])
        start = [dict(carrfreq=freq[i], codefreq=1.023e6, remcode=0.0, remcarr=0.0, buffloc=res[i]["buffloc"])
                 for i in range(2)] + [keep[2]]
        engine.trk_start_from_acq()
        assert engine.trk_get_state() == start
        engine.trk_set_state(keep)
        before = bytes(engine.loop_get()[2])
        engine.loop_start_from_acq()
        # the host path, the refined frequency in place of acqfreq
        for i in range(2):
            host.loop_set([host.loop_state(i, freq[i])], ch0=i)
        host.trk_set_state(start[:2])
        dl, hl = engine.loop_get(), host.loop_get()
        assert engine.trk_get_state() == host.trk_get_state() == start
        assert [bytes(x) for x in dl] == [bytes(x) for x in hl] and bytes(dl[2]) == before
        assert [l.acqfreq for l in dl[:2]] == freq and dl[0].cnt == 0 and dl[0].flagsync == 0
        # 200 periods: the oracle's loop from that state (channels 0 and 1), and the second engine
        ring = orc.make_ring(sig, nsig, nsig)
        track, bufflocs = [], []
        for i in range(2):
            o = orc.make_chan(HO_PRNS[i], dtype=2, f_sf=F4, f_if=0.0)
            o.acq.acqfreq = freq[i]
            o.carrfreq, o.codefreq, o.remcode, o.remcarr = freq[i], 1.023e6, 0.0, 0.0
            o.flagsync, o.synci, o.cnt = 0, 0, 0
            track.append(o)
            bufflocs.append(C.c_uint64(res[i]["buffloc"]))
        _check_against_oracle(orc, engine, track, ring, bufflocs, 200, 5)
        host.trk_run_loop(200)
        for a, b in zip(engine.trk_fetch() + engine.trk_fetch_log(), host.trk_fetch() + host.trk_fetch_log()):
            assert a.tobytes() == b.tobytes()
        assert [bytes(x) for x in engine.loop_get()] == [bytes(x) for x in host.loop_get()]
        assert engine.trk_get_state() == host.trk_get_state()
    finally:
        host.close()


# ---- 6. schedule -----------------------------------------------------------------------------------------------------
def test_schedule_cold_start_tracks_from_the_refined_frequency(gc, orc, synth, engine):
    """One cold start through gnsscorr_rx_step with a satellite 90 Hz off its bin centre: the channel reaches TRACK and
    its loop's acqfreq is the restatement's finefreq; a second channel with nref = 0 keeps its bin centre."""
    sc = fc.SCEN["iq4"]
    W, pairs, wants = fc.scenario(gc, orc, synth, "iq4")
    pairs = [pairs[0], pairs[3]]                                # PRN 3 at 600 - 90 Hz, PRN 22 at -200 + 90 Hz
    chans = [c for c, _ in pairs]
    engine.ring_create(1, 2, ec.granule(len(W), 2))
    engine.set_channels(chans)
    engine.loop_set([engine.loop_state(i, 0.0) for i in range(2)])
    engine.acq_set_refine([10, 0])
    engine.rx_start()
    first = 7 * fc.N4
    engine.ring_push_raw(1, W[:first], first)
    engine.rx_step(5)
    assert [s["state"] for s in engine.rx_status()] == [gc.CH_SEARCH] * 2
    engine.ring_push_raw(1, W[first:], len(W) - first)
    engine.rx_step(5)
    st = engine.rx_status()
    assert [s["state"] for s in st] == [gc.CH_TRACK] * 2 and [s["attempts"] for s in st] == [1, 1]
    for s, w in zip(st, (wants[0], wants[3])):
        ac.check_result(s["acq"], w, "rx")
    want = fc.fine_all(orc, pairs, W, len(W), [s["acq"] for s in st], [10, 0])
    fine = engine.acq_fetch_fine()
    ls = engine.loop_get()
    assert ls[0].acqfreq == want[0]["finefreq"] == fine[0]["finefreq"] != st[0]["acq"]["acqfreq"]
    assert abs(ls[0].acqfreq - (600.0 - 90.0)) < 25.0
    assert ls[1].acqfreq == st[1]["acq"]["acqfreq"] == fine[1]["finefreq"] and fine[1]["nref"] == 0
    _, ndone = engine.trk_fetch_log()
    assert np.all(ndone >= 1)


# ---- 7. fresh state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["iq4", "coh"])
def test_first_search_of_a_poisoned_engine(gc, orc, synth, name):
    """The first search of an engine whose buffers start out as 0xA5 gives the results of test 1."""
    e = gc.Engine(0)
    try:
        e.debug_poison(0xA5)
        _scenario_on_engine(e, gc, orc, synth, name, fc.nrefs(fc.SCEN[name])[1])
    finally:
        e.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_setting(gc, orc, synth, engine):
    """Every refusal of gnsscorr_acq_set_refine leaves the setting in place and names the channel; fetch_fine before a
    search is refused; set_channels resets every channel to 0 and applies the channels' own nref."""
    sc = fc.SCEN["iq4"]
    W, pairs, _ = fc.scenario(gc, orc, synth, "iq4")
    chans = [gc.Channel(c.prn, dtype=2, f_sf=F4, f_if=0.0, hband=1400, step=200, intg=i)
             for (c, _), i in zip(pairs, (10, 10, 4, 10, 10))]
    _load(engine, sc, W)
    with pytest.raises(gc.GnsscorrError):
        engine.acq_set_refine([2])                              # no channels yet
    with pytest.raises(gc.GnsscorrError):
        engine.acq_fetch_fine()
    engine.set_channels(chans)
    with pytest.raises(gc.GnsscorrError) as err:
        engine.acq_fetch_fine()                                 # no search yet
    assert "acq_fetch_fine" in str(err.value)
    setting = [10, 2, 4, 0, 7]
    engine.acq_set_refine(setting)
    bad = [([-1], 0), ([1], 1), ([11], 0), ([5], 2), ([21], 4),                 # < 0, 1, > intg, > intg 4, > MAXCOH
           ([2] * 6, 0), ([2], 5), ([2], -1), ([2, 2], 4), ([], 0),           # a range outside the table
           ([2, 2, 5, 2], 0)]                                                   # one bad entry: nothing is touched
    for nref, ch0 in bad:
        with pytest.raises(gc.GnsscorrError) as err:
            engine.acq_set_refine(nref, ch0=ch0)
        assert "acq_set_refine" in str(err.value)
        assert engine.acq_get_refine() == setting, (nref, ch0)
    with pytest.raises(gc.GnsscorrError) as err:
        engine.acq_set_refine([2, 2, 5], ch0=0)
    assert "channel 2" in str(err.value)
    twenty = [gc.Channel(3, dtype=2, f_sf=F4, f_if=0.0, hband=200, step=200, intg=25)]
    engine.set_channels(twenty)
    assert engine.acq_get_refine() == [0]
    engine.acq_set_refine([20])
    with pytest.raises(gc.GnsscorrError):
        engine.acq_set_refine([21])
    assert engine.acq_get_refine() == [20]
    engine.set_channels([gc.Channel(3, dtype=2, f_sf=F4, f_if=0.0, hband=1400, step=200, intg=10, nref=6),
                         gc.Channel(8, dtype=2, f_sf=F4, f_if=0.0, hband=1400, step=200, intg=10)])
    assert engine.acq_get_refine() == [6, 0] and engine.acq_get_refine(ch0=1, nch=1) == [0]
    engine.acq_run(len(W))
    fine = engine.acq_fetch_fine()
    assert [f["nref"] for f in fine] == [6, 0]
