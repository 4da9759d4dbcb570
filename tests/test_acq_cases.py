"""CPU checks of the acquisition scenarios of tests/test_gpu_acq_edges.py and of the oracle pieces they lean on:
the scenario builder puts the oracle's peak on the requested lag and bin, the decisions keep their margins, a ring
that wrapped gives the oracle what the unwrapped stream gives it, the window-by-window search equals one full
orc_sdracquisition(), and orc_checkacquisition() equals a numpy restatement of maxvd / meanvd."""
import ctypes as C
import math

import numpy as np
import pytest

import acq_cases as ac


def _oracle_all(orc, pairs, buf, ringlen, wrpos):
    return ac.run_oracles([lambda o=o: ac.oracle_acq(orc, o, buf, ringlen, wrpos) for o in pairs])


def _checkacq_numpy(P, ns, ctime, freq):
    """ref src/sdracq.c:71-95 with maxvd (element 0 seeds the maximum, first maximum wins) and meanvd
    (ref src/sdrcmn.c:461-497)."""
    nfreq, n = P.shape
    flat = P.ravel()
    maxi = 0
    for i in range(1, flat.size):
        if flat[maxi] < flat[i]:
            maxi = i
    codei, freqi = maxi % n, maxi // n
    out = ac.exclusion_mask(n, codei, ns)
    row = P[freqi]
    mx2 = row[0]
    for i in np.nonzero(out)[0]:
        if mx2 < row[i]:
            mx2 = row[i]
    with np.errstate(divide="ignore", invalid="ignore"):
        meanP = row[out].sum() / out.sum()
        cn0 = 10 * np.log10(flat[maxi] / meanP / ctime)
        peakr = flat[maxi] / mx2
    return codei, freqi, freq[freqi], float(cn0), float(peakr)


@pytest.mark.parametrize("peak", ["0", "1", "2ns", "n-1", "zeros"])
def test_checkacquisition_matches_numpy(orc, peak):
    n, ns, nfreq, ctime = 2048, 2, 3, 1e-3
    rng = np.random.default_rng(5)
    P = rng.uniform(1.0, 2.0, (nfreq, n))
    lag = {"0": 0, "1": 1, "2ns": 2 * ns, "n-1": n - 1, "zeros": 0}[peak]
    P[1, lag] = 40.0
    P[1, (lag + 1) % n] = 20.0          # inside the window: not the runner-up
    if peak == "1":
        P[1, 0] = 30.0                  # inside the window too, but element 0 seeds maxvd
    if peak == "zeros":
        P[:] = 0.0
    freq = np.array([-250.0, 0.0, 250.0])
    res = orc.AcqRes()
    acq = orc.lib().orc_checkacquisition(P.ctypes.data, n, nfreq, ns, ctime, freq.ctypes.data, C.byref(res))
    codei, freqi, f, cn0, peakr = _checkacq_numpy(P, ns, ctime, freq)
    assert (res.acqcodei, res.freqi, res.acqfreq) == (codei, freqi, f)
    if peak == "zeros":
        assert math.isnan(res.cn0) and math.isnan(cn0) and math.isnan(res.peakr) and math.isnan(peakr)
        assert (codei, freqi, acq) == (0, 0, 0)
        return
    assert abs(res.cn0 - cn0) <= 1e-12 * abs(cn0) and abs(res.peakr - peakr) <= 1e-12 * peakr
    assert acq == (peakr > 3.0)
    if peak in ("0", "1"):
        # element 0 lies in the window and seeds maxvd: at lag 0 the ratio is exactly 1
        assert codei == lag and res.peakr == (1.0 if lag == 0 else 40.0 / 30.0) and not acq


@pytest.mark.parametrize("rate", list(ac.D_RATES))
def test_builder_places_lags(gc, orc, synth, rate):
    """Case D's spans: the oracle's peak on every requested lag, margins kept, lag 0 as quirk Q3 says."""
    W, n, lags = ac.case_d_span(gc, synth, rate, 51)
    f_sf, intg = ac.D_RATES[rate], ac.D_GRID[2]
    prns = list(lags)
    ochs = [ac.grid(orc.make_chan(p, dtype=2, f_sf=f_sf), *ac.D_GRID) for p in prns]
    for p, w in zip(prns, _oracle_all(orc, ochs, W, len(W), len(W))):
        ac.check_margins(w, p)
        assert w["acqcodei"] == lags[p], (p, lags[p], w["acqcodei"])
        if lags[p] == 0:
            assert w["peakr"] == 1.0 and not w["flagacq"] and w["iters"] == intg and w["buffloc"] == intg * n


def test_builder_places_doppler_bins(gc, orc, synth):
    """Satellites at the centres of the first and last bin of a 9-bin grid land there."""
    f_sf, n = 16.368e6, 16368
    hband, step, intg = ac.C_GRID
    nf = 2 * (hband // step) + 1
    sats = [ac.sat_at(21, 100, n, f_sf, ac.bin_doppler(nf, step, 0), 48.0, mid=0, into=0.3),
            ac.sat_at(29, 16000, n, f_sf, ac.bin_doppler(nf, step, nf - 1), 48.0, mid=0, into=0.3)]
    W = ac.span(gc, synth, sats, n, intg, f_sf, 0.0, 2, 61)
    ochs = [ac.grid(orc.make_chan(p, dtype=2, f_sf=f_sf), *ac.C_GRID) for p in (21, 29)]
    wants = _oracle_all(orc, ochs, W, len(W), len(W))
    for w in wants:
        ac.check_margins(w)
    assert [(w["acqcodei"], w["freqi"]) for w in wants] == [(100, 0), (16000, nf - 1)]


@pytest.mark.parametrize("shape", list(ac.C_SHAPES))
def test_wrap_cases(gc, orc, synth, shape):
    """Case C: the margins, the weak channel decided in a middle iteration, and the oracle on the ring-ordered array
    equal to the oracle on the unwrapped stream for every ring length and wrap point (shown at the first; the span is
    the same in all of them)."""
    f_sf, f_if, dtype = ac.C_SHAPES[shape]
    W, n = ac.case_c_span(gc, synth, shape, 41)
    intg = ac.C_GRID[2]
    prns = (ac.C_STRONG, ac.C_WEAK, ac.C_ABSENT)
    ochs = [ac.grid(orc.make_chan(p, dtype=dtype, f_sf=f_sf, f_if=f_if), *ac.C_GRID) for p in prns]
    ref = _oracle_all(orc, ochs, W, len(W), len(W))
    for w in ref:
        ac.check_margins(w, shape)
    assert ref[0]["flagacq"] and ref[0]["iters"] == 1
    assert ref[1]["flagacq"] and 2 <= ref[1]["iters"] < intg
    assert not ref[2]["flagacq"] and ref[2]["iters"] == intg
    if dtype == 1:
        return              # (the wrap construction does not depend on the sample type)
    for ringlen in ac.ring_lengths(n, intg, dtype).values():
        for d in ac.wrap_points(n, intg).values():
            b0 = ringlen - d
            stream = np.concatenate([ac.noise(b0, dtype, d), W])
            wrpos = b0 + (intg + 1) * n
            buf = ac.ring_order(stream, ringlen, wrpos)
            assert np.array_equal(buf[0], W[d])          # ring index 0 holds span sample d
            got = _oracle_all(orc, ochs, buf, ringlen, wrpos)
            for g, w in zip(got, ref):
                assert g["buffloc"] - b0 == w["buffloc"]
                for k in ("flagacq", "iters", "acqcodei", "freqi", "acqfreq", "cn0", "peakr"):
                    assert g[k] == w[k], (ringlen, d, k)
                assert np.array_equal(g["P"], w["P"])


def test_window_by_window_equals_full_search(gc, orc, synth):
    """oracle_acq (orc_sdracquisition with intg 1 per window, the power kept) gives what one
    orc_sdracquisition(intg) gives: decided at iteration 1, in a middle iteration, and not at all."""
    shape = "16M_iq"
    f_sf, f_if, dtype = ac.C_SHAPES[shape]
    W, n = ac.case_c_span(gc, synth, shape, 41)
    for p in (ac.C_STRONG, ac.C_WEAK, ac.C_ABSENT):
        o = ac.grid(orc.make_chan(p, dtype=dtype, f_sf=f_sf, f_if=f_if), *ac.C_GRID)
        w = ac.oracle_acq(orc, o, W, len(W), len(W))
        o = ac.grid(orc.make_chan(p, dtype=dtype, f_sf=f_sf, f_if=f_if), *ac.C_GRID)
        xc = orc.codespectrum(o)
        o.xcode = xc.ctypes.data
        P = np.zeros(o.nfreq * n)
        it = C.c_int()
        ring = orc.make_ring(W, len(W), len(W))
        buffloc = orc.lib().orc_sdracquisition(C.byref(o), C.byref(ring), P.ctypes.data, C.byref(it))
        assert (w["flagacq"], w["iters"], w["buffloc"]) == (o.flagacq, it.value, buffloc)
        assert (w["acqcodei"], w["freqi"], w["acqfreq"], w["cn0"], w["peakr"]) == \
            (o.acq.acqcodei, o.acq.freqi, o.acq.acqfreq, o.acq.cn0, o.acq.peakr)
        assert np.array_equal(w["P"].ravel(), P)


def test_middle_iteration_spread(gc, orc, synth):
    """Case A: both spans keep their margins; the first is decided at three or more different middle iterations."""
    spreads = []
    for seed in ac.A_SEEDS:
        W = ac.case_a_span(gc, synth, seed)
        ochs = [orc.make_chan(p, dtype=2, f_sf=ac.A_F_SF) for p in ac.A_CHANS]
        wants = _oracle_all(orc, ochs, W, len(W), len(W))
        for p, w in zip(ac.A_CHANS, wants):
            ac.check_margins(w, (seed, p))
        assert wants[-2]["flagacq"] and wants[-2]["iters"] == 1
        assert not wants[-1]["flagacq"] and wants[-1]["iters"] == 10
        spreads.append({w["iters"] for w in wants if w["flagacq"] and 2 <= w["iters"] <= 9})
    assert len(spreads[0]) >= 3, spreads


def test_td_lags_matches_td_range(orc):
    """orc_pcorrelator_td_lags is orc_pcorrelator_td at a list of lags."""
    o = orc.make_chan(7, dtype=2, f_sf=2.048e6)
    n, m = o.nsamp, 2 * o.nsamp
    data = np.random.default_rng(3).integers(-60, 61, (m, 2), dtype=np.int8)
    freq = np.ascontiguousarray(np.ctypeslib.as_array(o.freq)[:3])
    code = np.ascontiguousarray(np.ctypeslib.as_array(o.code)[:o.clen])
    full = np.zeros(3 * n)
    orc.lib().orc_pcorrelator_td(data.ctypes.data, 2, o.ti, n, freq.ctypes.data, 3, m, code.ctypes.data, o.clen,
                                 o.ci, 0, n, full.ctypes.data)
    lags = np.array([0, 1, 5, 777, n - 1], np.int32)
    P = np.zeros(3 * len(lags))
    orc.lib().orc_pcorrelator_td_lags(data.ctypes.data, 2, o.ti, n, freq.ctypes.data, 3, m, code.ctypes.data,
                                      o.clen, o.ci, lags.ctypes.data, len(lags), P.ctypes.data)
    assert np.array_equal(P.reshape(3, -1), full.reshape(3, n)[:, lags])


@pytest.mark.parametrize("shape", list(ac.B_SHAPES))
def test_middle_iteration_spread_65536(gc, orc, synth, shape):
    """Case B: margins kept, three or more different middle iterations, the strong channel at 1, the absent one never."""
    f_sf, f_if, dtype = ac.B_SHAPES[shape]
    W, n = ac.case_b_span(gc, synth, shape)
    prns = ac.B_CHANS[shape]
    ochs = [ac.grid(orc.make_chan(p, dtype=dtype, f_sf=f_sf, f_if=f_if), *ac.B_GRID) for p in prns]
    wants = _oracle_all(orc, ochs, W, len(W), len(W))
    for p, w in zip(prns, wants):
        ac.check_margins(w, (shape, p))
    assert len({w["iters"] for w in wants if w["flagacq"] and 2 <= w["iters"] <= 9}) >= 3
    assert wants[-2]["flagacq"] and wants[-2]["iters"] == 1
    assert not wants[-1]["flagacq"] and wants[-1]["iters"] == 10


def test_mixed_grid_decisions(gc, orc, synth):
    """Case E: margins kept on every grid; the 3-iteration channel decided at iteration 2."""
    W = ac.case_a_span(gc, synth, ac.A_SEEDS[0])
    ochs = [ac.grid(orc.make_chan(p, dtype=2, f_sf=ac.A_F_SF), *g) for p, g in ac.E_CHANS]
    wants = _oracle_all(orc, ochs, W, len(W), len(W))
    for (p, _), w in zip(ac.E_CHANS, wants):
        ac.check_margins(w, p)
    assert [(w["flagacq"], w["iters"]) for w in wants] == [(1, 5), (1, 2), (0, 3), (0, 3), (1, 1), (0, 1)]
