"""Coherent integration over several code periods per search (gnsscorr_acq_set_coherent): a
restatement of its semantics on the host, and the scenarios of tests/test_acq_coh_host.py (which shows on the
restatement alone that each is decided with room) and tests/test_gpu_acq_coherent.py (which runs them on the device).
Helpers; not a conftest.

The restatement (`coh_acq`), for a channel with intg windows in G = intg/ncoh groups, n = nsamp, b0 = wrpos -
(intg+1)*n:
  1. group g covers ring samples [b0 + g*ncoh*n, b0 + g*ncoh*n + (ncoh+1)*n);
  2. per Doppler bin the span is wiped off by one literal mixcarr() call over its (ncoh+1)*n samples, phase 0 at the
     first one (orc_mixcarr_seq: integers I, Q);
  3. z[k] = sum_{j<ncoh} (I, Q)[j*n + k], k < 2n, in integers (numpy int64; |z| <= 20*2*32*128 < 2^24, so the
     conversion to the reference's float is exact);
  4. z * CSCALE/nfft, the forward transform, .conj(C), the inverse transform, |y|^2/nfft^2 added to the fp64 power:
     the reference's own scalings and transform length (ref src/sdrcmn.c:738-773, 228-251: orc_cpxcpx and orc_cpxconv
     with the code spectrum of orc_codespectrum), once per group, no normalisation by ncoh;
  5. checkacquisition()'s rules after every group (orc_checkacquisition on the summed power), the first passing group
     wins;
  6. iters = (g+1)*ncoh, buffloc = b0 + acqcodei (acquired) or b0 + intg*n, cn0 = 10 log10(maxP/meanP/(ncoh*ctime)),
     acqfreq the bin's frequency.
With ncoh = 1 every call is the one acq_cases.oracle_acq makes through orc_sdracquisition, so the two agree bit for bit.

`coh_power_td` is the same power without any transform: fp64 time-domain sums of z against the resampled code at chosen
lags, what the device's power array is held against element-wise (as acq_cases.power_td for ncoh = 1).
"""
import ctypes as C
import math

import numpy as np

import acq_cases as ac
from acq_cases import MARGIN, POWER_TOL, push_wrapping, ring_order, sat_at, span  # noqa: F401  (shared by import)

CSCALE = 1.0 / 32.0         # ref src/sdr.h (CSCALE), orc ORC_CSCALE


def _span_samples(ring_buf, ringlen, start, count):
    idx = (start + np.arange(count, dtype=np.int64)) % ringlen
    return np.ascontiguousarray(ring_buf[idx])


def group_sum(orc, o, ring_buf, ringlen, start, ncoh, freq):
    """Steps 1-3 for one bin: (zI, zQ) int64 arrays of 2n entries, and the span's wiped-off integers."""
    n = o.nsamp
    cnt = (ncoh + 1) * n
    win = _span_samples(ring_buf, ringlen, start, cnt)
    I = np.zeros(cnt + 64, np.int16)
    Q = np.zeros(cnt + 64, np.int16)
    orc.lib().orc_mixcarr_seq(win.ctypes.data, o.dtype, o.ti, cnt, float(freq), 0.0, I.ctypes.data, Q.ctypes.data)
    I = I[:cnt].astype(np.int64)
    Q = Q[:cnt].astype(np.int64)
    zI = np.zeros(2 * n, np.int64)
    zQ = np.zeros(2 * n, np.int64)
    for j in range(ncoh):
        zI += I[j * n:j * n + 2 * n]
        zQ += Q[j * n:j * n + 2 * n]
    return zI, zQ, I, Q


def _check(orc, o, P, ncoh):
    """checkacquisition() on the summed power; cn0 over the group's coherent time."""
    res = orc.AcqRes()
    freq = np.ascontiguousarray(np.ctypeslib.as_array(o.freq)[:o.nfreq])
    orc.lib().orc_checkacquisition(P.ctypes.data, o.nsamp, o.nfreq, o.nsampchip, o.ctime, freq.ctypes.data,
                                   C.byref(res))
    n = o.nsamp
    row = P.reshape(o.nfreq, n)[res.freqi]
    if ncoh == 1:
        cn0 = res.cn0
    else:
        # the sum in the reference's order (meanvd, ref src/sdrcmn.c:487-497), the division by ncoh*ctime
        out = ac.exclusion_mask(n, res.acqcodei, o.nsampchip)
        mean = 0.0
        for v in row[out]:
            mean += v
        mean /= int(out.sum())
        maxP = row[res.acqcodei]
        cn0 = 10 * math.log10(maxP / mean / (ncoh * o.ctime)) if mean > 0 and maxP > 0 else float("nan")
    return res, cn0


def coh_acq(orc, o, ring_buf, ringlen, wrpos, ncoh):
    """The restated search of oracle channel `o` with ncoh periods per group.  Returns what acq_cases.oracle_acq
    returns: dict(flagacq, iters, buffloc, acqcodei, freqi, acqfreq, cn0, peakr, P (nfreq, nsamp) at the deciding
    group, steps = [(peakr, acqcodei, freqi, lag gap, row gap)] per group up to the deciding one, b0), and groups."""
    n, intg, m = o.nsamp, o.intg, o.nfft
    assert ncoh >= 1 and intg % ncoh == 0 and m == 2 * n
    G = intg // ncoh
    xc = orc.codespectrum(o)
    freq = np.ctypeslib.as_array(o.freq)[:o.nfreq].copy()
    P = np.zeros(o.nfreq * n)
    b0 = wrpos - (intg + 1) * n
    dx = np.zeros(2 * m, np.float32)
    sc = np.float32(CSCALE / m)
    steps, res, cn0, acq = [], None, float("nan"), 0
    for g in range(G):
        start = b0 + g * ncoh * n
        for b in range(o.nfreq):
            zI, zQ, _, _ = group_sum(orc, o, ring_buf, ringlen, start, ncoh, freq[b])
            # cpxcpx (ref src/sdrcmn.c:185-195): integer * (float)scale, the sum converted once
            dx[0::2] = zI.astype(np.float32) * sc
            dx[1::2] = zQ.astype(np.float32) * sc
            orc.lib().orc_cpxconv(dx.ctypes.data, xc.ctypes.data, m, n, 1, P[b * n:].ctypes.data)
        res, cn0 = _check(orc, o, P, ncoh)
        steps.append((res.peakr, res.acqcodei, res.freqi) + ac.gaps(P.reshape(o.nfreq, n)))
        acq = int(res.acquired)
        if acq:
            break
    groups = len(steps)
    return dict(flagacq=acq, iters=groups * ncoh if acq else intg,
                buffloc=b0 + res.acqcodei if acq else b0 + intg * n,
                acqcodei=res.acqcodei, freqi=res.freqi, acqfreq=res.acqfreq, cn0=cn0, peakr=res.peakr,
                P=P.reshape(o.nfreq, n), steps=steps, b0=b0, groups=groups, ncoh=ncoh)


def coh_power_td(orc, o, ring_buf, ringlen, b0, groups, ncoh, lags):
    """fp64 time-domain power at `lags` in every bin, summed over groups 0..groups-1: |sum_j z[lag + j] rc[j]|^2 /
    (32 m)^2 with z the integer sum of step 3 and rc the resampled code: (nfreq, len(lags))."""
    n, m = o.nsamp, 2 * o.nsamp
    lags = np.asarray(lags, np.int64)
    code = np.ascontiguousarray(np.ctypeslib.as_array(o.code)[:o.clen])
    rc = np.zeros(n, np.int16)
    orc.lib().orc_rescode_seq(code.ctypes.data, o.clen, 0.0, 0, o.ci, n, rc.ctypes.data)
    rc = rc.astype(np.float64)
    freq = np.ctypeslib.as_array(o.freq)[:o.nfreq].copy()
    idx = lags[:, None] + np.arange(n)[None, :]
    P = np.zeros((o.nfreq, len(lags)))
    sc = 32.0 * m
    for g in range(groups):
        start = b0 + g * ncoh * n
        for b in range(o.nfreq):
            zI, zQ, _, _ = group_sum(orc, o, ring_buf, ringlen, start, ncoh, freq[b])
            sr = zI.astype(np.float64)[idx] @ rc         # integers below 2^53: exact
            si = zQ.astype(np.float64)[idx] @ rc
            P[b] += (sr * sr + si * si) / (sc * sc)
    return P


# ---- scenarios ------------------------------------------------------------------------------------------------------
# A scenario: one span of (intg+1)*n samples (intg the largest of its channels) with satellites placed by
# acq_cases.sat_at, and the channels searched on it.  sats: (prn, lag, doppler Hz, C/N0 dB-Hz, carrier phase[, sample
# from which the data bit is flipped]); chans: (prn, hband, step, intg, ncoh).  4.092 Msps (4 samples per chip, nsamp
# 4092) is the smallest shape the kernels take whole.  Dopplers sit on bin centres of every grid that searches them.
SCEN = {
    # 36 dB-Hz is the value the issue starts from; it separates the two searches on the literal LUT path for seeds
    # 0..3 alike (tests/test_acq_coh_host.py), so no 0.5 dB step was needed.  PRN 1, +1000 Hz, lag 1234: the pilot.
    "weak": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=2, sats=[(1, 1234, 1000.0, 36.0, 0.3)],
                 chans=[(1, 7000, 200, 10, 1), (1, 5000, 50, 10, 10)]),
    # one group of 10; groups of 5: a satellite that passes at group 1, one (negative Doppler: a carrier phase that
    # falls) that passes only at group 2, an absent PRN
    "iq10": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=4,
                 sats=[(9, 3210, 50.0, 40.0, 0.2), (7, 2345, 100.0, 45.0, 0.7), (11, 777, -200.0, 36.5, 1.9)],
                 chans=[(9, 200, 50, 10, 10), (7, 400, 100, 10, 5), (11, 400, 100, 10, 5), (5, 400, 100, 10, 5)]),
    # the weak satellite with its data bit flipped in the middle of the span: the 10 ms group loses the peak.  A
    # satellite strong enough (iq10's first, 40 dB-Hz) is still acquired, two bins off: the flip splits its line.
    "flip": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=2, sats=[(1, 1234, 1000.0, 36.0, 0.3, 5 * 4092 + 2046)],
                 chans=[(1, 5000, 50, 10, 10)]),
    "flip40": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=4, sats=[(9, 3210, 50.0, 40.0, 0.2, 5 * 4092 + 2046)],
                   chans=[(9, 200, 50, 10, 10)]),
    # real samples at an IF: the satellite in a bin below the IF centre
    "real": dict(f_sf=16.368e6, f_if=4.092e6, dtype=1, seed=6, sats=[(13, 9999, -250.0, 43.0, 1.0)],
                 chans=[(13, 1000, 250, 4, 2), (13, 1000, 250, 4, 4)]),
    # periods of 20000 samples: the 65536-point transform
    "m20": dict(f_sf=20e6, f_if=0.0, dtype=2, seed=7, sats=[(20, 12345, 250.0, 42.0, 2.0)],
                chans=[(20, 1000, 250, 4, 2)]),
    # ncoh 1 / 5 / 10 on grids of 71 / 141 / 201 bins with intg 10 / 10 / 20 on one ring
    "mixed": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=8,
                  sats=[(3, 100, 600.0, 46.0, 0.1), (8, 1500, -1000.0, 44.0, 0.9), (14, 3000, 400.0, 42.0, 1.7),
                        (22, 4000, -150.0, 41.0, 2.5)],
                  chans=[(3, 7000, 200, 10, 1), (8, 7000, 100, 10, 5), (14, 7000, 100, 10, 5), (22, 5000, 50, 20, 10)]),
}


def nsamp(sc):
    return int(sc["f_sf"] * 1e-3)


def max_intg(sc):
    return max(c[3] for c in sc["chans"])


def make_span(gc, synth, sc):
    """The scenario's span W, (max intg + 1)*n samples.  A satellite is exactly on its lag in the middle of W."""
    n, intg = nsamp(sc), max_intg(sc)
    sats = []
    for t in sc["sats"]:
        prn, lag, dop, cn0, ph = t[:5]
        a = sat_at(prn, lag, n, sc["f_sf"], dop, cn0, phase=ph, mid=intg // 2)
        if len(t) > 5:
            # the data bit flips at sample t[5]: a second copy, carrier turned by pi, takes over there
            b = dict(a)
            a["t_off"] = b["t_on"] = t[5] / sc["f_sf"]
            b["phase"] = a["phase"] + math.pi
            sats.append(b)
        sats.append(a)
    return span(gc, synth, sats, n, intg, sc["f_sf"], sc["f_if"], sc["dtype"], sc["seed"])


def pair(gc, orc, sc, chan):
    """(device Channel, oracle channel) of one entry of a scenario's chans."""
    prn, hband, step, intg, ncoh = chan
    c = gc.Channel(prn, dtype=sc["dtype"], f_sf=sc["f_sf"], f_if=sc["f_if"], hband=hband, step=step, intg=intg, ncoh=ncoh)
    o = ac.grid(orc.make_chan(prn, dtype=sc["dtype"], f_sf=sc["f_sf"], f_if=sc["f_if"]), hband, step, intg)
    assert o.nfreq == c.nfreq and np.array_equal(np.ctypeslib.as_array(o.freq)[:o.nfreq], c.freq)
    return c, o


_cache = {}


def scenario(gc, orc, synth, name):
    """(span W, [(Channel, oracle channel)], [restated result]) of a scenario, the ring being W itself and the search
    ending at its last sample: computed once per process."""
    if name not in _cache:
        sc = SCEN[name]
        W = make_span(gc, synth, sc)
        pairs = [pair(gc, orc, sc, ch) for ch in sc["chans"]]
        jobs = [lambda o=o, ch=ch: coh_acq(orc, o, W, len(W), len(W), ch[4]) for (_, o), ch in zip(pairs, sc["chans"])]
        _cache[name] = (W, pairs, ac.run_oracles(jobs))
    return _cache[name]
