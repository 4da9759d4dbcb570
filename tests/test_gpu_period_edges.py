"""Tracking and acquisition at the period lengths where the kernels change shape, against the CPU oracle (parity tests
proper, -m gpu).  Scenarios: tests/period_edge_cases.py, every length named after the line of the library that makes
it special; tests/test_period_edges_host.py shows on the oracle alone that each is what it claims to be.

Bars, none of them new: tracking sums, samples per period, batch sums and the chained state bit for bit
(tests/test_gpu_tracking.py); the closed loop teacher-forced as in tests/test_gpu_loop.py (integers bit for bit, filter
outputs to 1e-12); acquisition decisions identical to the oracle's, peakr and cn0 to 1e-4, the power arrays element-wise
to acq_cases.POWER_TOL of the row mean outside the exclusion window (tests/test_gpu_acq_edges.py) -- here over all nsamp
columns against the oracle's own power array, and at acq_cases.check_lags against the fp64 time-domain sum; the
refinement as tests/test_gpu_acq_fine.py."""
import ctypes as C

import numpy as np
import pytest

import acq_cases as ac
import acq_coh_cases as cc
import acq_edge_cases as ec
import period_edge_cases as pe

pytestmark = pytest.mark.gpu
EINVAL = -1
_ratios = []


# ---- helpers ---------------------------------------------------------------------------------------------------------
def _load_trk(engine, scenes):
    """The scenes' rings, channels and start states on one engine: (channels, oracle II, QQ, ns, final states)."""
    for sc in scenes:
        engine.ring_create(sc["ftype"], sc["dtype"], sc["nsamples"])
        engine.ring_push_raw(sc["ftype"], sc["data"], sc["nsamples"])
    chans = [c for sc in scenes for c in sc["chans"]]
    engine.set_channels(chans)
    engine.trk_set_state([st for sc in scenes for st in sc["states"]])
    return (chans, np.concatenate([sc["oII"] for sc in scenes]), np.concatenate([sc["oQQ"] for sc in scenes]),
            np.concatenate([sc["ons"] for sc in scenes]), [f for sc in scenes for f in sc["ofin"]])


def _run_batches(engine, nbatch=2, nper=3):
    """nbatch consecutive trk_run(nper): [(II, QQ, ns, sumI, sumQ)] and the final state."""
    out = []
    for _ in range(nbatch):
        engine.trk_run(nper)
        II, QQ, ns = engine.trk_fetch()
        sI, sQ = engine.trk_fetch_sums()
        out.append((II, QQ, ns, sI, sQ))
    return out, engine.trk_get_state()


def _check_batches(got, fin, oII, oQQ, ons, ofin, where, rows=None):
    """Two batches of three periods against the oracle's six: sums, samples per period and trk_fetch_sums bit for
    bit, the final remainders and positions equal.  rows: the channels of the engine that oII .. ofin speak of."""
    rows = range(oII.shape[0]) if rows is None else rows
    nper = got[0][0].shape[1]
    for b, (II, QQ, ns, sI, sQ) in enumerate(got):
        sl = slice(nper * b, nper * b + nper)
        for k, r in enumerate(rows):
            at = (where, "batch", b, "channel", r)
            assert np.array_equal(ns[r], ons[k, sl]), (at, ns[r], ons[k, sl])
            assert np.array_equal(II[r], oII[k, sl]) and np.array_equal(QQ[r], oQQ[k, sl]), at
            assert np.array_equal(sI[r], oII[k, sl].sum(axis=0)) and np.array_equal(sQ[r], oQQ[k, sl].sum(axis=0)), at
    for k, r in enumerate(rows):
        a, o = fin[r], ofin[k]
        assert (a["remcode"], a["remcarr"], a["buffloc"]) == (o["remcode"], o["remcarr"], o["buffloc"]), (where, r)


def _track_scenes(engine, scenes, where):
    chans, oII, oQQ, ons, ofin = _load_trk(engine, scenes)
    got, fin = _run_batches(engine)
    _check_batches(got, fin, oII, oQQ, ons, ofin, where)
    return got, fin


def _same(a, b, where):
    """Two engines' batches and final states, bit for bit."""
    for x, y in zip(a[0], b[0]):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes(), where
    assert a[1] == b[1], where


# ---- B. batched tracking at the segment and edge-table boundaries -----------------------------------------------------
@pytest.mark.parametrize("dtype,name,nsamp", [(d, k, n) for d in (1, 2) for k, n in pe.trk_lengths(d)])
def test_tracking_on_either_side_of_a_boundary(gc, orc, engine, dtype, name, nsamp):
    """Four channels from _setup's mix of start states, two batches of three periods, five taps, real and IQ samples,
    at: 1023 samples (one per chip), the last length of one segment and the first of two, 32768, the last of two and the
    first of three, 65000 (three segments, still an edge table), 65535 and 65536 (no table: the replica positions pass
    uint16), 131072 (six) and 262144 (eleven segments of GC_MAXR rounds each)."""
    assert dict(pe.trk_lengths(dtype))[name] == nsamp
    _track_scenes(engine, [pe.length_scene(gc, orc, dtype, nsamp)], (dtype, name))


@pytest.mark.parametrize("dtype", [1, 2])
def test_table_and_no_table_units_inside_one_batch(gc, orc, engine, dtype):
    """65532 samples: a channel whose first period has 65531 replica positions (a table) and whose later ones have 65543
    and more (none, their closing chip edge beyond 65535), and a channel whose periods have 65534 and 65535 in turn."""
    _track_scenes(engine, [pe.straddle_scene(gc, orc, dtype)], ("straddle", dtype))


@pytest.mark.parametrize("dtype", [1, 2])
def test_codes_with_and_without_an_edge_table_in_one_launch(gc, orc, engine, dtype):
    """Codes handed in through gnsscorr_chan_t.code at 16368 samples: alternating every chip (more edges than the table
    holds), constant (none) and a PRN, in one channel set."""
    _track_scenes(engine, [pe.codes_scene(gc, orc, dtype)], ("codes", dtype))


@pytest.mark.parametrize("dtype", [2, 1])
def test_full_scale_samples_33_taps_262144(gc, orc, engine, dtype):
    """The largest sums the int32 accumulators hold: 262144 samples per period, every one an int8 extreme of the sign
    opposite to the prompt replica, 33 taps out to 64 samples -- for IQ samples 0.97 of (262144 + 100) x 128 x
    max(|cos32| + |sin32|), which the table the device mixes with keeps below 2^31."""
    cos32, sin32 = pe.device_lut(gc)
    hcos, hsin = pe.header_lut()
    assert np.array_equal(cos32, hcos) and np.array_equal(sin32, hsin)
    assert pe.accumulator_bound(cos32, sin32) < 2 ** 31
    _track_scenes(engine, [pe.full_scale_scene(gc, orc, dtype)], ("full scale", dtype))


@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("dtype", [1, 2])
def test_short_channels_beside_long_ones(gc, orc, engine, dtype, swapped):
    """2048-sample channels on one ring beside 262144-sample channels on the other: the context's eleven segments leave
    ten empty for every unit of the short channels.  Against the oracle, and the short channels bit for bit against
    the same channels alone on a fresh engine."""
    short, long_ = pe.mixed_scenes(gc, orc, dtype, swapped)
    got, fin = _track_scenes(engine, [short, long_], ("mixed", dtype, swapped))
    alone = gc.Engine(0)
    try:
        ref = _track_scenes(alone, [short], ("short alone", dtype, swapped))
    finally:
        alone.close()
    k = len(short["chans"])
    for (II, QQ, ns, sI, sQ), (rII, rQQ, rns, rsI, rsQ) in zip(got, ref[0]):
        for u, v in ((II, rII), (QQ, rQQ), (ns, rns), (sI, rsI), (sQ, rsQ)):
            assert u[:k].tobytes() == v.tobytes()
    assert fin[:k] == ref[1]


@pytest.mark.parametrize("case", ["65536", "mixed"])
def test_poisoned_engine_gives_the_plain_engines_results(gc, orc, engine, case):
    """An engine whose buffers start out as 0xA5 (empty segments' partial sums, rounds and edge tables included) against
    a plain one: 65536 samples, and the short channels beside the long ones."""
    scenes = [pe.length_scene(gc, orc, 2, 65536)] if case == "65536" else list(pe.mixed_scenes(gc, orc, 2, False))
    plain = _track_scenes(engine, scenes, ("plain", case))
    other = gc.Engine(0)
    try:
        other.debug_poison(0xA5)
        _same(_track_scenes(other, scenes, ("poisoned", case)), plain, case)
    finally:
        other.close()


# ---- C. closed loop and drop-ins --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsamp,flagsync", [(49037, 0), (65536, 0), (65536, 1), (262144, 0)])
def test_closed_loop_at_three_and_eleven_segments(gc, orc, engine, nsamp, flagsync):
    """trk_run_loop over 30 periods at 49037 (the first IQ length of three segments), 65536 (no edge table; filter update
    every period, and every ten with ten-period sums once the bit edge is known) and 262144 samples (eleven segments),
    teacher-forced as tests/test_gpu_loop.py: three channels from random start states.  (Before the tail kernel built
    every round of a period -- it stopped at 64, one per lane -- the 65536 cases failed in their first period, prompt
    sum -4628.84375 against the oracle's -4622.46875, after 25.8 s; the 262144 case was refused as too long.)"""
    from test_gpu_loop import _random_states_case
    f_sf, f_if = pe.front_end(nsamp, 2)
    pe.check_nsamp(gc.Channel(1, dtype=2, f_sf=f_sf, f_if=f_if), orc.make_chan(1, dtype=2, f_sf=f_sf, f_if=f_if), nsamp)
    assert pe.nseg(2, nsamp) == {49037: 3, 65536: 3, 262144: 11}[nsamp]
    _random_states_case(gc, orc, engine, 4000 + nsamp % 997 + flagsync, 2, f_if, f_sf, pe.TAPS5, flagsync, nper=30,
                        nch=3, chunks=(30,), ring_granule=8)


@pytest.mark.parametrize("dtype", [2, 1])
def test_correlator_symbol_grows_and_shrinks(gc, orc, dtype):
    """correlator() on one thread at n = 16368, 65536, 262144 and 16368 again: its segment buffers grow twice and are
    then used for a single segment; sums and remainders bit for bit."""
    L = gc.lib()
    rng = np.random.default_rng(50 + dtype)
    code, crate = gc.gencode(5, gc.CTYPE_L1CA)
    code16 = code.astype(np.int16)
    s = np.array([3, 6, 9], np.int32)
    for n in (16368, 65536, 262144, 16368):
        f_sf, f_if = pe.front_end(n, dtype)
        data = rng.integers(-100, 101, size=n * dtype, dtype=np.int8)
        freq, phi0, coff = f_if + float(rng.uniform(-4000, 4000)), float(rng.uniform(0, 6)), float(rng.uniform(0, 1000))
        II, QQ = np.zeros(7), np.zeros(7)
        remc, remp = C.c_double(), C.c_double()
        L.correlator(data.ctypes.data, dtype, 1 / f_sf, n, freq, phi0, crate + 1.5, coff, s.ctypes.data, 3,
                     II.ctypes.data, QQ.ctypes.data, C.byref(remc), C.byref(remp), code16.ctypes.data, 1023)
        oII, oQQ, orc_c, orc_p = orc.correlator(data, dtype, 1 / f_sf, n, freq, phi0, crate + 1.5, coff, s, code16)
        assert np.any(oII) and np.array_equal(II, oII) and np.array_equal(QQ, oQQ), (dtype, n)
        assert remc.value == orc_c and remp.value == orc_p, (dtype, n)


# ---- A. acquisition at the transform boundaries -----------------------------------------------------------------------
def _load_acq(engine, sc, ftype=1):
    W = sc["W"]
    engine.ring_create(ftype, sc["dtype"], ec.granule(len(W), sc["dtype"]))
    engine.ring_push_raw(ftype, W, len(W))
    assert engine.ring_wrpos(ftype) == len(W)


def _check_acq(engine, orc, sc, where, td=None, first=0):
    """The last search's results and power arrays of channels first .. first + 3 against the scenario's oracle results:
    check_result's bars, and every cell of acq_power against the oracle's power array.  td(o, w, lags): the fp64
    time-domain power at the check lags, held against the device's likewise."""
    res = engine.acq_fetch()[first:first + 4]
    n = sc["n"]
    jobs = []
    for i, ((c, o), r, w) in enumerate(zip(sc["pairs"], res, sc["wants"])):
        at = (where, c.prn)
        ac.check_result(r, w, at)
        P = engine.acq_power(first + i)
        assert P.shape == w["P"].shape == (c.nfreq, n) and c.nfreq == 5, at
        ratio = pe.power_ratio_full(P, w["P"], w["acqcodei"], c.nsampchip)
        _ratios.append(ratio)
        print(f"power {where} prn {c.prn} acq {w['flagacq']} iters {w['iters']}: max |dP|/meanP over all cells {ratio:.3g} "
              f"(largest so far {max(_ratios):.3g})")
        assert ratio <= ac.POWER_TOL, (at, ratio)
        for cn0, PP, d in ((r["cn0"], P, r), (w["cn0"], w["P"], w)):
            want = ac._cn0_restated(PP, d["acqcodei"], d["freqi"], c.nsampchip, c.ctime * w.get("ncoh", 1))
            assert abs(cn0 - want) <= 1e-9 * abs(want), (at, cn0, want)
        if i == 1:                                              # the satellite at the last lag
            assert w["acqcodei"] == n - 1 and int(np.argmax(P[r["freqi"]])) == n - 1 and P[r["freqi"], n - 1] == P.max(), at
        if td is not None and i < 3:
            lags = ac.check_lags(o, w["acqcodei"], np.random.default_rng(i))
            jobs.append((i, P, lags, lambda o=o, w=w, lags=lags: td(o, w, lags)))
    for (i, P, lags, _), ptd in zip(jobs, ac.run_oracles([j[3] for j in jobs])):
        w, c = sc["wants"][i], sc["pairs"][i][0]
        ratio = ac.power_ratio(P, ptd, lags, w["P"], w["acqcodei"], c.nsampchip)
        _ratios.append(ratio)
        print(f"power {where} prn {c.prn}: max |dP|/meanP against the time-domain sum {ratio:.3g}")
        assert ratio <= ac.POWER_TOL, (where, c.prn, ratio)
    return res


def _search(engine, gc, orc, synth, name, where=None):
    sc = pe.acq_scene(gc, orc, synth, name)
    _load_acq(engine, sc)
    engine.set_channels([c for c, _ in sc["pairs"]])
    engine.acq_run(sc["wrpos"])
    W = sc["W"]
    res = _check_acq(engine, orc, sc, where or name,
                     td=lambda o, w, lags: ac.power_td(orc, o, W, len(W), w["b0"], w["iters"], lags))
    return sc, res


@pytest.mark.parametrize("name", pe.PLAIN_SCEN)
def test_acquisition_at_the_transform_boundaries(gc, orc, synth, engine, name):
    """1023 samples (nsampchip 1, the narrowest exclusion window), 16384 (the 32768-point transform without padding),
    16385 (the first length of the 65536-point one) and 32768 (that one without padding), IQ samples and, at 16384 and
    32768, real samples at an IF: peaks at lag 0, at lag nsamp - 1 and 2 nsampchip before the end on the outer bin,
    and an absent PRN, on five bins with intg 2."""
    sc, res = _search(engine, gc, orc, synth, name)
    assert [r["flagacq"] for r in res] == [0, int(sc["n"] == 1023), 1, 0]
    assert [r["acqcodei"] for r in res[:3]] == list(pe.acq_lags(sc["n"]))


def test_16384_alone_takes_the_32768_point_transform(gc, orc, synth, engine):
    """The 16384-sample channels alone on an engine, and beside a 16385-sample channel on ring 2 that forces the set
    onto the 65536-point transform (as test_mixed_rates_force_65536): the search integers identical, cn0 and peakr
    within 1e-4, both against the oracle -- and the two power arrays within POWER_TOL of each other but not the same
    bits, which they would be had the lone engine taken the 65536-point transform too."""
    sc, res1 = _search(engine, gc, orc, synth, "iq16384", "16384 alone")
    sb = pe.acq_scene(gc, orc, synth, "iq16385")
    e2 = gc.Engine(0)
    try:
        # each ring's own write position ends its search: the span's first three periods on ring 1, all three on ring 2
        e2.ring_create(1, 2, ec.granule(len(sc["W"]), 2))
        e2.ring_push_raw(1, sc["W"][:sc["wrpos"]], sc["wrpos"])
        _load_acq(e2, sb, ftype=2)
        assert (e2.ring_wrpos(1), e2.ring_wrpos(2)) == (sc["wrpos"], sb["wrpos"])
        c2, _ = pe.acq_pairs(gc, orc, "iq16385", ftype=2)[2]
        e2.set_channels([c for c, _ in sc["pairs"]] + [c2])
        e2.acq_run(0)
        res2 = e2.acq_fetch()
        ac.check_result(res2[4], sb["wants"][2], "16385 on ring 2")
        for i, (a, b, w) in enumerate(zip(res1, res2, sc["wants"])):
            for k in ("flagacq", "iters", "buffloc", "acqcodei", "freqi", "acqfreq"):
                assert a[k] == b[k], (i, k)
            for k in ("peakr", "cn0"):
                assert abs(a[k] - b[k]) <= 1e-4 * abs(b[k]), (i, k)
            ac.check_result(b, w, ("forced", i))
            P1, P2 = engine.acq_power(i), e2.acq_power(i)
            assert pe.power_ratio_full(P2, w["P"], w["acqcodei"], sc["pairs"][i][0].nsampchip) <= ac.POWER_TOL, i
            assert pe.power_ratio_full(P1, P2, w["acqcodei"], sc["pairs"][i][0].nsampchip) <= ac.POWER_TOL, i
            assert not np.array_equal(P1, P2), i
    finally:
        e2.close()


@pytest.mark.parametrize("name", pe.COH_SCEN)
def test_coherent_groups_at_16384_and_32768(gc, orc, synth, engine, name):
    """ncoh 2 with intg 4 against acq_coh_cases.coh_acq."""
    sc = pe.coh_scene(gc, orc, synth, name)
    _load_acq(engine, sc)
    engine.set_channels([c for c, _ in sc["pairs"]])
    assert engine.acq_get_coherent() == [2] * 4
    engine.acq_run(sc["wrpos"])
    W = sc["W"]
    res = _check_acq(engine, orc, sc, ("coherent", name),
                     td=lambda o, w, lags: cc.coh_power_td(orc, o, W, len(W), w["b0"], w["groups"], 2, lags))
    assert [r["flagacq"] for r in res] == [0, 0, 1, 0] and res[2]["iters"] == 2


def test_refinement_at_32768(gc, orc, synth, engine):
    """nref 2 at 32768 samples against acq_fine_cases.fine_freq: the prompt sums of the longest period a search takes,
    bit for bit, the other bars as tests/test_gpu_acq_fine.py; the search itself unmoved."""
    from test_gpu_acq_fine import _check_fine
    sc = pe.acq_scene(gc, orc, synth, "iq32768")
    _load_acq(engine, sc)
    engine.set_channels([c for c, _ in sc["pairs"]])
    engine.acq_set_refine([2] * 4)
    engine.acq_run(sc["wrpos"])
    res, fine, P = _check_fine(engine, orc, sc["pairs"], sc["W"], len(sc["W"]), 2, "iq32768")
    for (c, _), r, w in zip(sc["pairs"], res, sc["wants"]):
        ac.check_result(r, w, ("refine", c.prn))
    assert [f["nref"] for f in fine] == [0, 0, 2, 0] and P[2, :2].any() and not P[[0, 1, 3]].any()
    assert abs(fine[2]["finefreq"] - pe.ACQ_DOP[2]) <= 1.0 / (4.0 * 2 * 1e-3)


def test_handover_at_32768_tracks_three_periods(gc, orc, synth, engine):
    """trk_start_from_acq after the 32768-sample search, then three tracked periods of every channel -- the acquired one
    from its hand-over state, the others from the states they were given -- against the oracle, bit for bit."""
    from test_gpu_tracking import _oracle_run
    sc = pe.acq_scene(gc, orc, synth, "iq32768")
    n, W = sc["n"], sc["W"]
    _load_acq(engine, sc)
    chans = [c for c, _ in sc["pairs"]]
    engine.set_channels(chans)
    keep = [dict(carrfreq=900.0 + i, codefreq=1.023e6 + 0.25 * i, remcode=0.125 * (i + 1), remcarr=0.5 + i,
                 buffloc=3001 + 17 * i) for i in range(4)]
    engine.trk_set_state(keep)
    engine.acq_run(sc["wrpos"])
    res = engine.acq_fetch()
    for (c, _), r, w in zip(sc["pairs"], res, sc["wants"]):
        ac.check_result(r, w, ("handover", c.prn))
    engine.trk_start_from_acq()
    start = engine.trk_get_state()
    want = list(keep)
    want[2] = dict(carrfreq=res[2]["acqfreq"], codefreq=1.023e6, remcode=0.0, remcarr=0.0, buffloc=res[2]["buffloc"])
    assert start == want and res[2]["buffloc"] == n - 64
    engine.trk_run(3)
    II, QQ, ns = engine.trk_fetch()
    fe = pe.acq_front("iq32768")
    ochs = [orc.make_chan(c.prn, **fe) for c in chans]
    oII, oQQ, ons, ofin = _oracle_run(orc, ochs, start, W, len(W), len(W), 3)
    assert np.array_equal(ns, ons) and np.array_equal(II, oII) and np.array_equal(QQ, oQQ)
    for a, o in zip(engine.trk_get_state(), ofin):
        assert (a["remcode"], a["remcarr"], a["buffloc"]) == (o["remcode"], o["remcarr"], o["buffloc"])


def test_search_is_refused_above_32768_and_the_engine_goes_on(gc, orc, synth, engine):
    """A 32769-sample channel: set_channels takes it and a batch of three periods tracks bit for bit; acq_run fails
    with GNSSCORR_EINVAL and names the transform it would need.  A 32768-sample set on the same engine then searches
    as on a fresh one."""
    from test_gpu_tracking import _oracle_run
    sc = pe.acq_scene(gc, orc, synth, "iq32768")
    W = sc["W"]
    _load_acq(engine, sc)
    f_sf, f_if = pe.front_end(32769, 2)
    c, o = ec.pair(gc, orc, dict(dtype=2, f_sf=f_sf, f_if=f_if), (9, 400, 200, 2, 1, 0))
    pe.check_nsamp(c, o, 32769)
    engine.set_channels([c])
    st = [dict(carrfreq=1234.5, codefreq=c.crate - 1.25, remcode=0.375, remcarr=2.5, buffloc=1003)]
    engine.trk_set_state(st)
    engine.trk_run(3)
    II, QQ, ns = engine.trk_fetch()
    oII, oQQ, ons, ofin = _oracle_run(orc, [orc.make_chan(9, dtype=2, f_sf=f_sf, f_if=f_if)], st, W, len(W), len(W), 3)
    assert np.array_equal(ns, ons) and np.array_equal(II, oII) and np.array_equal(QQ, oQQ) and ons.max() > 32768
    L = gc.lib()
    assert L.gnsscorr_acq_run(engine.h, 3 * 32769) == EINVAL
    msg = L.gnsscorr_last_error().decode()
    assert "nsamp 32769" in msg and "needs an FFT longer than 65536" in msg, msg
    engine.set_channels([c for c, _ in sc["pairs"]])
    engine.acq_run(sc["wrpos"])
    _check_acq(engine, orc, sc, "after the refusal")


@pytest.mark.parametrize("bad", [0, 262145])
def test_set_channels_refuses_nsamp_outside_1_262144(gc, orc, engine, bad):
    """nsamp 0 and 262145 are refused, the channel is named, and the set in force goes on tracking bit for bit."""
    sc = pe.length_scene(gc, orc, 2, 1023)
    chans, oII, oQQ, ons, ofin = _load_trk(engine, [sc])
    engine.trk_run(3)
    first = engine.trk_fetch() + engine.trk_fetch_sums()
    wrong = gc.Channel(5, dtype=2, f_sf=1.023e6, f_if=0.0)
    wrong.nsamp = bad
    with pytest.raises(gc.GnsscorrError) as err:
        engine.set_channels([chans[0], wrong])
    assert "channel 1" in str(err.value) and f"nsamp {bad} (1..262144 supported)" in str(err.value)
    assert gc.lib().gnsscorr_num_channels(engine.h) == len(chans)
    assert engine.channels == chans
    engine.trk_run(3)
    second = engine.trk_fetch() + engine.trk_fetch_sums()
    _check_batches([first, second], engine.trk_get_state(), oII, oQQ, ons, ofin, ("refused", bad))
