"""Acquisition scenarios with a known answer, and the checks that go with them (helpers of
tests/test_gpu_acq_edges.py and tests/test_acq_cases.py; not a conftest).

A scenario is a search span W of (intg+1)*nsamp samples: the samples that sdracquisition() looks at for a write
position wrpos are W = stream[wrpos - (intg+1)*nsamp : wrpos] (ref src/sdracq.c:24-32).  Satellites are placed in W
so that their code periods start at a chosen lag of every window and their Doppler lies at the centre of a chosen
bin; what precedes W in the stream is noise the search never reads.

The oracle is run window by window (`oracle_acq`): orc_sdracquisition() with intg = 1 and the write position of
window k, on a power array that keeps its sum, is the k-th iteration of the full search (its getbuff, pcorrelator and
checkacquisition on the power summed over windows 0..k), and gives the decision of every iteration on the way.
"""
import ctypes as C
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F_CF = 1575.42e6
MARGIN = 1e-3           # relative gap a decision needs to be safe from fp32 rounding
POWER_TOL = 1e-4        # |P_gpu - P_td| <= POWER_TOL * (row mean outside the exclusion window)


def sat_at(prn, lag, nsamp, f_sf, doppler, cn0, phase=0.3, mid=None, into=None):
    """A satellite whose code periods start at sample `lag` (mod nsamp) of W, i.e. the oracle's peak at that lag.
    The code runs at crate*(1 + doppler/f_cf) (synth.make_if), so it slides by doppler/f_cf; it is exactly on the
    lag at the start of period `mid` of W (default 5: the middle of a 10-iteration span), the slide is split to both
    sides.
    into: how far (in samples) sample `lag` lies into the period's first chip there; the default, 1e-3 chip, is for
    Dopplers whose slide over the span stays well below that (zero); a satellite at several kHz wants a fraction of a
    sample and `mid` at the window that decides it."""
    crate = 1.023e6
    rate = crate * (1.0 + doppler / F_CF)
    m = mid if mid is not None else 5
    s_ref = lag + m * nsamp
    # sample s_ref is chip 0, not the last chip of the period before
    off = 1e-3 if into is None else into * crate / f_sf
    cph = (off - rate * s_ref / f_sf) % 1023.0
    return dict(prn=prn, doppler=float(doppler), codephase=float(cph), cn0=float(cn0), phase=float(phase))


def bin_doppler(nfreq, step, b):
    """The Doppler at the centre of bin b of a grid of nfreq bins, step Hz apart (ref src/sdrinit.c:633-635)."""
    return float((b - (nfreq - 1) // 2) * step)


def span(gc, synth, sats, nsamp, intg, f_sf, f_if, dtype, seed, noise_sigma=8.0):
    codes = {s["prn"]: gc.gencode(s["prn"], gc.CTYPE_L1CA) for s in sats}
    return synth.make_if(codes, (intg + 1) * nsamp, f_sf=f_sf, f_if=f_if, dtype=dtype, sats=sats, seed=seed,
                         noise_sigma=noise_sigma)


def noise(n, dtype, seed, sigma=8.0):
    rng = np.random.default_rng(seed)
    x = np.clip(np.rint(rng.normal(0.0, sigma, (n, 2) if dtype == 2 else n)), -127, 127)
    return x.astype(np.int8)


def ring_order(stream, ringlen, wrpos):
    """The device ring after the stream's first wrpos samples went in: absolute sample p at index p % ringlen."""
    shape = (ringlen,) + stream.shape[1:]
    r = np.zeros(shape, np.int8)
    p = np.arange(max(0, wrpos - ringlen), wrpos)
    r[p % ringlen] = stream[p]
    return r


def push_wrapping(engine, ftype, stream, wrpos, ringlen, npieces=3):
    """The first wrpos samples of the stream into ring `ftype` in npieces (>= 2) pushes of at most ringlen."""
    npieces = max(npieces, 2, -(-wrpos // ringlen))
    cuts = np.linspace(0, wrpos, npieces + 1).astype(np.int64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert b - a <= ringlen
        engine.ring_push_raw(ftype, np.ascontiguousarray(stream[a:b]), int(b - a))


def grid(o, hband, step, intg):
    """Give an oracle channel the acquisition grid of Channel(hband=, step=, intg=)."""
    o.intg = intg
    o.nfreq = 2 * (hband // step) + 1
    for i in range(o.nfreq):
        o.freq[i] = o.f_if + (i - (o.nfreq - 1) // 2) * float(step) + o.foffset
    return o


def oracle_acq(orc, o, ring_buf, ringlen, wrpos):
    """The search of oracle channel `o` (its xcode set here) over ring_buf, window by window.
    Returns dict(flagacq, iters, buffloc, acqcodei, freqi, acqfreq, cn0, peakr, P (nfreq, nsamp) at the deciding
    iteration, steps = [(peakr, acqcodei, freqi, lag gap, row gap)] per iteration up to the deciding one)."""
    n, intg = o.nsamp, o.intg
    xc = orc.codespectrum(o)
    o.xcode = xc.ctypes.data
    P = np.zeros(o.nfreq * n)
    it = C.c_int()
    b0 = wrpos - (intg + 1) * n
    steps = []
    o.intg = 1
    try:
        for k in range(intg):
            o.flagacq = 0
            ring = orc.make_ring(ring_buf, ringlen, b0 + (k + 2) * n)
            orc.lib().orc_sdracquisition(C.byref(o), C.byref(ring), P.ctypes.data, C.byref(it))
            steps.append((o.acq.peakr, o.acq.acqcodei, o.acq.freqi) + gaps(P.reshape(o.nfreq, n)))
            if o.flagacq:
                break
    finally:
        o.intg = intg
        o.xcode = None
    acq = o.flagacq
    return dict(flagacq=acq, iters=len(steps), buffloc=b0 + o.acq.acqcodei if acq else b0 + intg * n,
                acqcodei=o.acq.acqcodei, freqi=o.acq.freqi, acqfreq=o.acq.acqfreq, cn0=o.acq.cn0, peakr=o.acq.peakr,
                P=P.reshape(o.nfreq, n), steps=steps, b0=b0)


def run_oracles(jobs, workers=16):
    """jobs: callables; run side by side (the oracle releases the GIL; its FFT tables are per thread)."""
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(lambda f: f(), jobs))


def gaps(P):
    """(winning lag vs the runner-up of its row, winning row vs the next best row), relative to the winner."""
    rmax = P.max(axis=1)
    fi = int(np.argmax(rmax))
    row = np.sort(P[fi])
    top = row[-1]
    if top <= 0:
        return (0.0, 0.0)
    rows = np.sort(rmax)
    return (float((top - row[-2]) / top), float((top - rows[-2]) / top) if len(rows) > 1 else 1.0)


def check_margins(res, where=""):
    """Every iteration up to the deciding one: lag and row decisions MARGIN apart, peak ratio MARGIN*3 off ACQTH."""
    for k, (peakr, _, _, glag, grow) in enumerate(res["steps"]):
        assert glag >= MARGIN, (where, k, "lag", glag)
        assert grow >= MARGIN, (where, k, "row", grow)
        assert abs(peakr - 3.0) >= MARGIN * 3.0, (where, k, "peakr", peakr)


def exclusion_mask(nsamp, codei, nsampchip):
    """True outside codei +- 2*nsampchip (wrapping), as checkacquisition() (ref src/sdracq.c:81-84)."""
    s, e = codei - 2 * nsampchip, codei + 2 * nsampchip
    s, e = s + nsamp if s < 0 else s, e - nsamp if e >= nsamp else e
    i = np.arange(nsamp)
    return ((i < s) | (i > e)) if s <= e else ((i < s) & (i > e))


def _cn0_restated(P, codei, freqi, nsampchip, ctime):
    """checkacquisition()'s C/N0 (ref src/sdracq.c:71-95): the peak over the mean of its Doppler row outside
    codei +- 2*nsampchip (wrapping), with an exactly rounded sum.  The peak ratio and the 1e-4 bar on cn0 cannot see
    that window's width at these shapes (one more sample per side moves cn0 by ~2e-5 relative): this can."""
    nsamp = P.shape[1]
    out = exclusion_mask(nsamp, codei, nsampchip)
    meanP = math.fsum(P[freqi][out]) / int(out.sum())
    return 10 * math.log10(P[freqi, codei] / meanP / ctime)


def check_lags(o, codei, rng):
    """Lags the element-wise check looks at: the peak +- (2*nsampchip + 2), 0..3, nsamp-4..nsamp-1, 256 random."""
    n = o.nsamp
    d = 2 * o.nsampchip + 2
    lags = {(codei - d) % n, (codei + d) % n, codei % n, 0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1}
    lags |= set(rng.integers(0, n, 256).tolist())
    return np.array(sorted(lags), np.int32)


def power_td(orc, o, ring_buf, ringlen, b0, iters, lags):
    """fp64 time-domain power of oracle channel `o` at `lags` in every bin, summed over windows 0..iters-1 the way
    the device sums them: (nfreq, len(lags))."""
    n, m = o.nsamp, 2 * o.nsamp
    lags = np.ascontiguousarray(lags, np.int32)
    P = np.zeros(o.nfreq * len(lags))
    code = np.ascontiguousarray(np.ctypeslib.as_array(o.code)[:o.clen])
    freq = np.ascontiguousarray(np.ctypeslib.as_array(o.freq)[:o.nfreq])
    for k in range(iters):
        idx = (b0 + k * n + np.arange(m)) % ringlen
        win = np.ascontiguousarray(ring_buf[idx])
        orc.lib().orc_pcorrelator_td_lags(win.ctypes.data, o.dtype, o.ti, n, freq.ctypes.data, o.nfreq, m,
                                          code.ctypes.data, o.clen, o.ci, lags.ctypes.data, len(lags), P.ctypes.data)
    return P.reshape(o.nfreq, len(lags))


def power_ratio(Pdev, Ptd, lags, Pref, codei, nsampchip):
    """max over bins and lags of |P_dev - P_td| / (row mean of Pref outside codei's exclusion window)."""
    mask = exclusion_mask(Pref.shape[1], codei, nsampchip)
    mean = Pref[:, mask].mean(axis=1)
    assert np.all(mean > 0)
    return float(np.max(np.abs(Pdev[:, lags] - Ptd) / mean[:, None]))


# ---- the scenarios of tests/test_gpu_acq_edges.py (their oracle margins are checked in tests/test_acq_cases.py)

# A: one 16.368 Msps IQ grid, C/N0s the oracle decides at different middle iterations; two spans (two acq_run calls)
A_F_SF, A_N = 16.368e6, 16368
A_PRNS = [4, 7, 9, 12, 14, 17, 19, 22, 25]           # satellites in the spans
A_CN0 = [39.5, 40.0, 40.5, 41.0, 41.5, 42.0, 41.5, 41.0, 40.5]
A_STRONG, A_ABSENT = 28, 5
A_CHANS = [4, 7, 9, 12, 17, 19, 22, A_STRONG, A_ABSENT]    # the searched channels
A_SEEDS = (1003, 3)                                         # noise of the first and of the second span


def case_a_sats(seed=3):
    """Dopplers on whole kHz: bin centres of the 200, 250 and 500 Hz grids alike."""
    rng = np.random.default_rng(seed)
    sats = [sat_at(p, int(rng.integers(0, A_N)), A_N, A_F_SF, 1000.0 * int(rng.integers(-3, 4)), c,
                   phase=float(rng.uniform(0, 6))) for p, c in zip(A_PRNS, A_CN0)]
    sats.append(sat_at(A_STRONG, int(rng.integers(0, A_N)), A_N, A_F_SF, 1000.0, 50.0))
    return sats


def case_a_span(gc, synth, seed):
    return span(gc, synth, case_a_sats(), A_N, 10, A_F_SF, 0.0, 2, seed)


# B: middle iterations on the 65536-point path (acq_corr64: no early exit, acq_final's loop decides), 26 Msps IQ and
# 20 Msps real at a 4 MHz IF, on a 31-bin grid
B_SHAPES = {"26M_iq": (26e6, 0.0, 2), "20M_real_if4M": (20e6, 4.0e6, 1)}
B_GRID = (3000, 200, 10)
B_PRNS = [3, 8, 13, 18, 23, 26, 29]
B_CN0 = {"26M_iq": [39.5, 40.0, 40.5, 41.0, 41.5, 42.0, 40.5], "20M_real_if4M": [39.5, 40.0, 40.5, 41.0, 41.5, 42.0, 40.5]}
B_STRONG = 30
B_CHANS = {"26M_iq": [3, 8, 13, 18, 23, 26, 29, B_STRONG, 10],        # the searched channels: the last one absent
           "20M_real_if4M": [3, 8, 18, 23, 26, 29, B_STRONG, 2]}
B_SEED = {"26M_iq": 21, "20M_real_if4M": 22}


def case_b_span(gc, synth, shape):
    f_sf, f_if, dtype = B_SHAPES[shape]
    n = int(f_sf * 1e-3)
    rng = np.random.default_rng(B_SEED[shape])
    sats = [sat_at(p, int(rng.integers(0, n)), n, f_sf, 1000.0 * int(rng.integers(-3, 4)), c,
                   phase=float(rng.uniform(0, 6))) for p, c in zip(B_PRNS, B_CN0[shape])]
    sats.append(sat_at(B_STRONG, int(rng.integers(0, n)), n, f_sf, -2000.0, 50.0))
    return span(gc, synth, sats, n, 10, f_sf, f_if, dtype, B_SEED[shape]), n


# E: one engine, one ring, channels whose grids differ in nfreq (71, 13, 9) and intg (10, 3, 1) over case A's first
# span: (prn, (hband, step, intg))
E_CHANS = [(7, (7000, 200, 10)), (17, (3000, 500, 3)), (12, (3000, 500, 3)), (A_ABSENT, (3000, 500, 3)),
           (A_STRONG, (1000, 250, 1)), (19, (1000, 250, 1))]


# C: ring wrap; a 9-bin grid keeps the oracle cheap, one weak satellite decided in a middle iteration
C_SHAPES = {"16M_real_if4M": (16.368e6, 4.092e6, 1), "16M_iq": (16.368e6, 0.0, 2),
            "26M_real_if4M": (26e6, 4.092e6, 1), "26M_iq": (26e6, 0.0, 2)}
C_GRID = (1000, 250, 10)            # hband, step, intg
C_STRONG, C_WEAK, C_ABSENT = 6, 11, 5
C_WEAK_CN0 = {"16M_real_if4M": 41.0, "16M_iq": 40.0, "26M_real_if4M": 41.0, "26M_iq": 40.0}


def case_c_span(gc, synth, shape, seed):
    f_sf, f_if, dtype = C_SHAPES[shape]
    n = int(f_sf * 1e-3)
    rng = np.random.default_rng(seed)
    sats = [sat_at(C_STRONG, int(rng.integers(0, n)), n, f_sf, 500.0, 48.0),
            sat_at(C_WEAK, int(rng.integers(0, n)), n, f_sf, -250.0, C_WEAK_CN0[shape], phase=1.1)]
    return span(gc, synth, sats, n, C_GRID[2], f_sf, f_if, dtype, seed), n


def wrap_points(n, intg):
    """Offsets from the span's first sample at which the ring wraps: inside the first window, an iteration's first
    sample, the second half of the last window, one sample before wrpos."""
    return {"first_window": n // 2 + 101, "iteration_start": 3 * n, "last_window": intg * n + n // 2 + 77,
            "before_wrpos": (intg + 1) * n - 1}


def ring_lengths(n, intg, dtype):
    """(intg+1)*nsamp exactly, and 12345 samples more rounded up to the ring's 16-byte granule."""
    g = 16 // dtype
    return {"exact": (intg + 1) * n, "plus12345": -(-((intg + 1) * n + 12345) // g) * g}


# D: peaks at the lags where checkacquisition()'s exclusion window wraps or touches an end
D_RATES = {"16M": 16.368e6, "2M": 2.048e6, "26M": 26e6}
D_GRID = (500, 250, 4)
D_PRNS = [1, 3, 5, 8, 10, 13, 15, 20, 24, 27]


def d_lags(n, ns):
    return sorted({0, 1, ns - 1, ns, 2 * ns - 1, 2 * ns, 2 * ns + 1, n - 2 * ns - 1, n - 2 * ns, n - 1})


def case_d_span(gc, synth, rate, seed):
    f_sf = D_RATES[rate]
    n = int(f_sf * 1e-3)
    ns = n // 1023
    lags = d_lags(n, ns)
    sats = [sat_at(p, lag, n, f_sf, 0.0, 50.0, phase=0.4 * i) for i, (p, lag) in enumerate(zip(D_PRNS, lags))]
    return span(gc, synth, sats, n, D_GRID[2], f_sf, 0.0, 2, seed), n, dict(zip(D_PRNS, lags))


def check_result(r, want, where=""):
    """Device result r (acq_fetch) against the oracle's (oracle_acq): decisions identical, peakr and cn0 to 1e-4;
    NaN only where the oracle has NaN."""
    for k in ("flagacq", "iters", "buffloc", "acqcodei", "freqi", "acqfreq"):
        assert r[k] == want[k], (where, k, r[k], want[k])
    for k in ("peakr", "cn0"):
        a, b = r[k], want[k]
        if math.isnan(b):
            assert math.isnan(a), (where, k, a, b)
        else:
            assert not math.isnan(a) and abs(a - b) <= 1e-4 * abs(b), (where, k, a, b)
