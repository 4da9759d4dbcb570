"""Bit-edge hypotheses for coherent groups (gnsscorr_acq_set_bitedge): a restatement of their
semantics on the host, and the scenarios of tests/test_acq_edge_host.py (which shows on the restatement alone that
each is decided with room) and tests/test_gpu_acq_bitedge.py (which runs them on the device).  Helpers; not a conftest.

The restatement (`edge_acq`) is acq_coh_cases.coh_acq with, per group and Doppler bin:
  1./2. the span and its one mixcarr() wipe-off (acq_coh_cases.group_sum: the integers I, Q of the (ncoh+1)*n samples);
  3.  per hypothesis h in {0, estep, 2 estep, ...}, h < ncoh:  z_h[k] = sum_{j<ncoh} s(h,j) (I, Q)[j*n + k], k < 2n,
      s(h,j) = -1 when h > 0 and j >= h, else +1, in int64;
  4.  z_h * CSCALE/nfft, the forward transform, .conj(C), the inverse transform, pw_h[k] = |y_h[k]|^2/nfft^2
      (orc_cpxconv without summing), the reference's scalings and transform length;
  5.  row rule: h* = the hypothesis with the largest max_{k<n} pw_h[k], the lowest h on ties; P[bin] += pw_{h*};
  6.  checkacquisition()'s rules on P after every group (acq_coh_cases._check), the first passing group wins; iters,
      buffloc, acqfreq, cn0 as coh_acq; edge = h* of the deciding group's best row (-1: not acquired, or estep 0).
With estep = 0 there is one hypothesis, h = 0, and every call is the one coh_acq makes: bit for bit the same.

`edge_power_td` is the fp64 time-domain power of the hypotheses the restatement chose, what the device's power array is
held against element-wise.
"""
import numpy as np

import acq_cases as ac
import acq_coh_cases as cc
from acq_cases import MARGIN, POWER_TOL  # noqa: F401  (shared by import)

TIE_CAP = 0.05          # share of a channel's rows whose two best hypotheses may lie within MARGIN of each other


def hyps(ncoh, estep):
    return list(range(0, ncoh, estep)) if estep > 0 else [0]


def signed_sums(I, Q, n, ncoh, hs):
    """Step 3 from the span's wiped-off integers: [(zI, zQ)] per hypothesis of hs."""
    wI = [I[j * n:j * n + 2 * n] for j in range(ncoh)]
    wQ = [Q[j * n:j * n + 2 * n] for j in range(ncoh)]
    out = []
    for h in hs:
        zI = np.zeros(2 * n, np.int64)
        zQ = np.zeros(2 * n, np.int64)
        for j in range(ncoh):
            if h > 0 and j >= h:
                zI -= wI[j]
                zQ -= wQ[j]
            else:
                zI += wI[j]
                zQ += wQ[j]
        out.append((zI, zQ))
    return out


def edge_acq(orc, o, ring_buf, ringlen, wrpos, ncoh, estep):
    """The restated search of oracle channel `o`.  Returns coh_acq's dict and: edge; hsel = per group the chosen h* per
    row (int array nfreq); hgap = per group the relative gap between the two best hypothesis maxima per row (1.0 with a
    single hypothesis); hs = the hypotheses."""
    n, intg, m = o.nsamp, o.intg, o.nfft
    assert ncoh >= 1 and intg % ncoh == 0 and m == 2 * n
    assert estep == 0 or (ncoh >= 2 and 1 <= estep < ncoh)
    hs = hyps(ncoh, estep)
    G = intg // ncoh
    xc = orc.codespectrum(o)
    freq = np.ctypeslib.as_array(o.freq)[:o.nfreq].copy()
    P = np.zeros(o.nfreq * n)
    b0 = wrpos - (intg + 1) * n
    dx = np.zeros(2 * m, np.float32)
    sc = np.float32(cc.CSCALE / m)
    pw = np.zeros(n)
    steps, hsel, hgap, res, cn0, acq = [], [], [], None, float("nan"), 0
    for g in range(G):
        start = b0 + g * ncoh * n
        sel = np.zeros(o.nfreq, np.int32)
        gap = np.ones(o.nfreq)
        for b in range(o.nfreq):
            _, _, I, Q = cc.group_sum(orc, o, ring_buf, ringlen, start, ncoh, freq[b])
            best, bmax, maxes = None, -1.0, []
            for h, (zI, zQ) in zip(hs, signed_sums(I, Q, n, ncoh, hs)):
                dx[0::2] = zI.astype(np.float32) * sc
                dx[1::2] = zQ.astype(np.float32) * sc
                orc.lib().orc_cpxconv(dx.ctypes.data, xc.ctypes.data, m, n, 0, pw.ctypes.data)
                mx = float(pw.max())
                maxes.append(mx)
                if mx > bmax:                   # strict: the lowest h on ties
                    bmax, best, sel[b] = mx, pw.copy(), h
            P[b * n:(b + 1) * n] += best
            if len(maxes) > 1:
                top = sorted(maxes)
                gap[b] = (top[-1] - top[-2]) / top[-1]
        hsel.append(sel)
        hgap.append(gap)
        res, cn0 = cc._check(orc, o, P, ncoh)
        steps.append((res.peakr, res.acqcodei, res.freqi) + ac.gaps(P.reshape(o.nfreq, n)))
        acq = int(res.acquired)
        if acq:
            break
    groups = len(steps)
    return dict(flagacq=acq, iters=groups * ncoh if acq else intg,
                buffloc=b0 + res.acqcodei if acq else b0 + intg * n,
                acqcodei=res.acqcodei, freqi=res.freqi, acqfreq=res.acqfreq, cn0=cn0, peakr=res.peakr,
                P=P.reshape(o.nfreq, n), steps=steps, b0=b0, groups=groups, ncoh=ncoh, estep=estep, hs=hs,
                hsel=hsel, hgap=hgap, edge=int(hsel[-1][res.freqi]) if acq and estep > 0 else -1)


def edge_power_td(orc, o, ring_buf, ringlen, b0, groups, ncoh, hsel, lags):
    """fp64 time-domain power at `lags` in every bin, summed over groups 0..groups-1, of the hypothesis hsel[g][bin]:
    |sum_j z_h[lag + j] rc[j]|^2 / (32 m)^2 with rc the resampled code: (nfreq, len(lags))."""
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
            _, _, I, Q = cc.group_sum(orc, o, ring_buf, ringlen, start, ncoh, freq[b])
            ((zI, zQ),) = signed_sums(I, Q, n, ncoh, [int(hsel[g][b])])
            sr = zI.astype(np.float64)[idx] @ rc         # integers below 2^53: exact
            si = zQ.astype(np.float64)[idx] @ rc
            P[b] += (sr * sr + si * si) / (sc * sc)
    return P


def tied_rows(res):
    """Rows (bins) that had, in some group up to the deciding one, their two best hypotheses within MARGIN."""
    tied = np.zeros(len(res["hgap"][0]), bool)
    for gap in res["hgap"]:
        tied |= gap < MARGIN
    return tied


def check_margins(res, where=""):
    """The conditions on a device test's input: after every group the winning lag leads by MARGIN, the winning row by
    2*MARGIN (a row that ties on its hypothesis moves its maximum by up to MARGIN), the peak ratio is 3*MARGIN off the
    threshold; the deciding row's two best hypotheses are MARGIN apart in every group, and at most TIE_CAP of the rows
    have theirs within MARGIN."""
    for k, (peakr, _, fi, glag, grow) in enumerate(res["steps"]):
        assert glag >= MARGIN, (where, k, "lag", glag)
        assert grow >= 2 * MARGIN, (where, k, "row", grow)
        assert abs(peakr - 3.0) >= MARGIN * 3.0, (where, k, "peakr", peakr)
        assert res["hgap"][k][fi] >= MARGIN, (where, k, "hypotheses of the best row", res["hgap"][k][fi])
    tied = tied_rows(res)
    assert not tied[res["freqi"]], (where, "deciding row ties")
    assert tied.mean() <= TIE_CAP, (where, "tied rows", int(tied.sum()), len(tied))


# ---- scenarios ------------------------------------------------------------------------------------------------------
# As acq_coh_cases.SCEN; chans: (prn, hband, step, intg, ncoh, estep).  A flip sits at lag + h*nsamp of the span: the
# satellite's own period boundary h, where the halves of an unhypothesised sum cancel most.
N4 = 4092


def _flip(lag, h, n=N4):
    return lag + h * n


SCEN = {
    # the pilot: PRN 1, +1000 Hz, lag 1234, 36 dB-Hz, the bit flipped on its fifth period boundary; estep 0 / 1 / 2
    "edge36": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=2, sats=[(1, 1234, 1000.0, 36.0, 0.3, _flip(1234, 5))],
                   chans=[(1, 5000, 50, 10, 10, 0), (1, 5000, 50, 10, 10, 1), (1, 5000, 50, 10, 10, 2)]),
    # 9-bin grids, one group of 10, estep 1, 40 to 42 dB-Hz: edges at 1 and at 9, none, a flip in mid-period (sample
    # 5.5 * nsamp of the span: the satellite of acq_coh_cases' flip40), an absent PRN.  Lags 2345, 3000, 3210: the
    # element-wise power bar is in units of the row's noise mean, and the fp32 transforms err at a peak by r * (the
    # cell's own value), r between 2e-7 and 1.7e-6 depending on the lag -- measured on the search *without* hypotheses,
    # 1.7e-6 at lags 1500 / 1501, 2e-7 .. 3e-7 at 2345, 3000 and 3210 -- so a peak 100 times the mean
    # meets the bar only where r < 1e-6, with or without this feature
    "edges40": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=54,
                    sats=[(22, 2345, -150.0, 41.0, 2.6, _flip(2345, 1)), (7, 2345, 100.0, 42.0, 0.7, _flip(2345, 9)),
                          (11, 3000, -100.0, 41.0, 1.9), (9, 3210, 50.0, 40.0, 0.2, 5 * N4 + 2046)],
                    chans=[(22, 200, 50, 10, 10, 1), (7, 200, 50, 10, 10, 1), (11, 200, 50, 10, 10, 1),
                           (9, 200, 50, 10, 10, 1), (5, 200, 50, 10, 10, 1)]),
    # groups of 5, the bit edge at span period 3: group 0 chooses 3, group 1 chooses 0.  One satellite passes at group
    # 1, one near 36.5 dB-Hz only at group 2 (two differently chosen rows added into P), an absent PRN
    "groups5": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=4,
                    sats=[(7, 2345, 100.0, 45.0, 0.7, _flip(2345, 3)), (11, 777, -200.0, 36.5, 1.9, _flip(777, 3))],
                    chans=[(7, 400, 100, 10, 5, 1), (11, 400, 100, 10, 5, 1), (5, 400, 100, 10, 5, 1)]),
    # estep 2: an edge on a hypothesis (4) and one between two (5)
    "step2": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=5,
                  sats=[(9, 3210, 50.0, 45.0, 0.2, _flip(3210, 4)), (7, 2345, -100.0, 45.0, 0.7, _flip(2345, 5))],
                  chans=[(9, 200, 50, 10, 10, 2), (7, 200, 50, 10, 10, 2)]),
    # real samples at an IF, nsamp 16368 (still the 32768-point transform), one group of 4, the edge at 2
    "real": dict(f_sf=16.368e6, f_if=4.092e6, dtype=1, seed=6,
                 sats=[(13, 9999, -250.0, 43.0, 1.0, _flip(9999, 2, 16368))],
                 chans=[(13, 1000, 250, 4, 4, 1)]),
    # a mixed list on one ring: ncoh 1, ncoh 5 without hypotheses, ncoh 5 with estep 1 (edge at 2 of its first group),
    # ncoh 10 with estep 5 on intg 20 (edge at 5 of its first group): grids of 10, 2, 2 x 5 and 2 x 2 slots.  The two
    # satellites whose power arrays are checked sit at lags 3000 and 3210 (see edges40)
    "mixed": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=8,
                  sats=[(3, 100, 600.0, 46.0, 0.1), (8, 1500, -1000.0, 44.0, 0.9),
                        (14, 3000, 400.0, 44.0, 1.7, _flip(3000, 12)), (22, 3210, -150.0, 42.0, 2.5, _flip(3210, 5))],
                  chans=[(3, 2000, 200, 10, 1, 0), (8, 2000, 100, 10, 5, 0), (14, 2000, 100, 10, 5, 1),
                         (22, 1500, 50, 20, 10, 5)]),
}


def pair(gc, orc, sc, chan):
    """(device Channel, oracle channel) of one entry of a scenario's chans."""
    c, o = cc.pair(gc, orc, sc, chan[:5])
    c.estep = chan[5]
    return c, o


_cache = {}


def scenario(gc, orc, synth, name):
    """(span W, [(Channel, oracle channel)], [restated result]) of a scenario, the ring being W itself and the search
    ending at its last sample: computed once per process."""
    if name not in _cache:
        sc = SCEN[name]
        W = cc.make_span(gc, synth, sc)
        pairs = [pair(gc, orc, sc, ch) for ch in sc["chans"]]
        jobs = [lambda o=o, ch=ch: edge_acq(orc, o, W, len(W), len(W), ch[4], ch[5])
                for (_, o), ch in zip(pairs, sc["chans"])]
        _cache[name] = (W, pairs, ac.run_oracles(jobs))
    return _cache[name]
