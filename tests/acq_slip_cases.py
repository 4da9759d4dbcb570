"""Code-Doppler compensation across the groups of a search (gnsscorr_acq_set_codedoppler): a restatement
of its semantics on the host, and the scenarios of tests/test_acq_slip_host.py (which shows on the restatement alone
that each is decided with room) and tests/test_gpu_acq_slip.py (which runs them on the device).  Helpers; not a conftest.

The restatement (`slip_acq`) is acq_coh_cases.coh_acq (with bit-edge hypotheses: acq_edge_cases.edge_acq) with the start
of step 1 moved: for a channel with G = intg/ncoh groups, n = nsamp, bins freq[b] and the carrier f_cf, in Python floats
(IEEE doubles) and in this order,
    dop    = (freq[b] - f_if) - foffset
    x      = (dop / f_cf) * float(g * ncoh * n)
    s(b,g) = -round(x)                  (round-half-even; s(b,0) = 0)
    back   = max(0, max s(b,g))
    b0     = wrpos - back - (intg+1)*n
and group g of bin b covers the (ncoh+1)*n ring samples from b0 + g*ncoh*n + s(b,g) on.  Everything else is the coherent
search's.  f_cf = 0: no shifts, back = 0, every call is the one coh_acq (edge_acq) makes.

`slip_power_td` is the same power without any transform, the start moved in the same way.

Spans come from synth.make_if with the scenario's own f_cf, which compresses the code by 1 + fd/f_cf; an f_cf far below
L1 compresses time (the kernel sees only the table).  No x of a scenario lies within HALF_GUARD of a half-integer
(`shifts` asserts it): the device's table and this one cannot differ by a rounding.
"""
import math

import numpy as np

import acq_cases as ac
import acq_coh_cases as cc
import acq_edge_cases as ec
from acq_cases import MARGIN, POWER_TOL  # noqa: F401  (shared by import)

HALF_GUARD = 1e-6
L1 = 1575.42e6


def shifts(freq, f_if, foffset, f_cf, G, ncoh, n):
    """(s int32 [nfreq][G], back) of a channel; f_cf 0: zeros."""
    s = np.zeros((len(freq), G), np.int32)
    if f_cf == 0:
        return s, 0
    for b in range(len(freq)):
        for g in range(G):
            dop = (float(freq[b]) - f_if) - foffset
            x = (dop / f_cf) * float(g * ncoh * n)
            assert abs(abs(x - math.floor(x)) - 0.5) > HALF_GUARD, ("x on a half-integer", b, g, x)
            s[b, g] = -round(x)
    return s, max(0, int(s.max()))


def chan_shifts(o, ncoh, f_cf):
    freq = np.ctypeslib.as_array(o.freq)[:o.nfreq]
    return shifts(freq, o.f_if, o.foffset, f_cf, o.intg // ncoh, ncoh, o.nsamp)


def slip_acq(orc, o, ring_buf, ringlen, wrpos, ncoh, f_cf, estep=0):
    """The restated search of oracle channel `o`.  Returns coh_acq's dict (estep > 0: edge_acq's, with edge, hsel, hgap,
    hs) and: back, shifts."""
    n, intg, m = o.nsamp, o.intg, o.nfft
    assert ncoh >= 1 and intg % ncoh == 0 and m == 2 * n
    assert estep == 0 or (ncoh >= 2 and 1 <= estep < ncoh)
    hs = ec.hyps(ncoh, estep)
    G = intg // ncoh
    sh, back = chan_shifts(o, ncoh, f_cf)
    xc = orc.codespectrum(o)
    freq = np.ctypeslib.as_array(o.freq)[:o.nfreq].copy()
    P = np.zeros(o.nfreq * n)
    b0 = wrpos - back - (intg + 1) * n
    dx = np.zeros(2 * m, np.float32)
    sc = np.float32(cc.CSCALE / m)
    pw = np.zeros(n)
    steps, hsel, hgap, res, cn0, acq = [], [], [], None, float("nan"), 0
    for g in range(G):
        sel = np.zeros(o.nfreq, np.int32)
        gap = np.ones(o.nfreq)
        for b in range(o.nfreq):
            start = b0 + g * ncoh * n + int(sh[b, g])
            if estep == 0:
                zI, zQ, _, _ = cc.group_sum(orc, o, ring_buf, ringlen, start, ncoh, freq[b])
                dx[0::2] = zI.astype(np.float32) * sc
                dx[1::2] = zQ.astype(np.float32) * sc
                orc.lib().orc_cpxconv(dx.ctypes.data, xc.ctypes.data, m, n, 1, P[b * n:].ctypes.data)
                continue
            _, _, I, Q = cc.group_sum(orc, o, ring_buf, ringlen, start, ncoh, freq[b])
            best, bmax, maxes = None, -1.0, []
            for h, (zI, zQ) in zip(hs, ec.signed_sums(I, Q, n, ncoh, hs)):
                dx[0::2] = zI.astype(np.float32) * sc
                dx[1::2] = zQ.astype(np.float32) * sc
                orc.lib().orc_cpxconv(dx.ctypes.data, xc.ctypes.data, m, n, 0, pw.ctypes.data)
                mx = float(pw.max())
                maxes.append(mx)
                if mx > bmax:                   # strict: the lowest h on ties
                    bmax, best, sel[b] = mx, pw.copy(), h
            P[b * n:(b + 1) * n] += best
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
    out = dict(flagacq=acq, iters=groups * ncoh if acq else intg,
               buffloc=b0 + res.acqcodei if acq else b0 + intg * n,
               acqcodei=res.acqcodei, freqi=res.freqi, acqfreq=res.acqfreq, cn0=cn0, peakr=res.peakr,
               P=P.reshape(o.nfreq, n), steps=steps, b0=b0, groups=groups, ncoh=ncoh, back=back, shifts=sh)
    if estep > 0:
        out.update(estep=estep, hs=hs, hsel=hsel, hgap=hgap, edge=int(hsel[-1][res.freqi]) if acq else -1)
    return out


def slip_power_td(orc, o, ring_buf, ringlen, b0, groups, ncoh, sh, lags, hsel=None):
    """fp64 time-domain power at `lags` in every bin, summed over groups 0..groups-1 (of the hypothesis hsel[g][bin] where
    given), each group's span started sh[bin][g] samples later: (nfreq, len(lags))."""
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
        for b in range(o.nfreq):
            start = b0 + g * ncoh * n + int(sh[b, g])
            zI, zQ, I, Q = cc.group_sum(orc, o, ring_buf, ringlen, start, ncoh, freq[b])
            if hsel is not None:
                ((zI, zQ),) = ec.signed_sums(I, Q, n, ncoh, [int(hsel[g][b])])
            sr = zI.astype(np.float64)[idx] @ rc         # integers below 2^53: exact
            si = zQ.astype(np.float64)[idx] @ rc
            P[b] += (sr * sr + si * si) / (sc * sc)
    return P


# ---- scenarios ------------------------------------------------------------------------------------------------------
# A scenario: one span W of (intg + 1)*n + back samples (back the largest of its channels; all of a scenario's channels
# have one intg) synthesised with the scenario's f_cf, and the channels searched on it, the search ending at W's last
# sample.  sats: (prn, lag, doppler Hz, C/N0 dB-Hz, carrier phase[, span period at whose start -- in the satellite's own
# frame -- the data bit flips]): the satellite's code periods start half a sample before sample lag of the *first*
# channel's search frame (b0 + lag + k*n) in the middle of group 0, and walk from there.  chans: (prn, hband, step, intg,
# ncoh, estep, f_cf of the compensation or 0).  Dopplers sit on bin centres.
DRIFT_CN0 = 33.5        # dB-Hz; found on the restatement (tests/test_acq_slip_host.py says how)
F41 = 41e6
SCEN = {
    # the peak walks 3.5 samples (0.87 chip) over the 8 groups and 0.5 sample inside one: the uncompensated search
    # (second channel) smears it
    "drift": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=2, f_cf=F41, sats=[(1, 1234, 1000.0, DRIFT_CN0, 0.3)],
                  chans=[(1, 1000, 500, 40, 5, 0, F41), (1, 1000, 500, 40, 5, 0, 0.0)]),
    # negative Doppler: later groups start later, back = 3
    "neg": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=3, f_cf=F41, sats=[(7, 2345, -1000.0, DRIFT_CN0 + 1.0, 1.1)],
                chans=[(7, 1000, 500, 40, 5, 0, F41), (5, 1000, 500, 40, 5, 0, F41)]),
    # the real constant: 200 periods in ten groups of 20, bins at -5, 0, +5 kHz, shifts up to +-2; an absent PRN runs
    # all ten groups
    "l1": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=5, f_cf=L1,
               sats=[(9, 3210, 5000.0, 27.0, 0.2), (14, 3000, -5000.0, 27.0, 1.7)],
               chans=[(9, 5000, 5000, 200, 20, 0, L1), (14, 5000, 5000, 200, 20, 0, L1), (6, 5000, 5000, 200, 20, 0, L1)]),
    # drift's shape with every bit-edge hypothesis, the bit flipped at span period 7 (group 1, h = 2)
    "edge": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=6, f_cf=F41, sats=[(1, 1234, 1000.0, DRIFT_CN0, 0.3, 7)],
                 chans=[(1, 1000, 500, 40, 5, 1, F41)]),
    # periods of 20000 samples: the 65536-point transform; shifts up to 12 samples at the grid's edges, 3 at the satellite
    "m20": dict(f_sf=20e6, f_if=0.0, dtype=2, seed=7, f_cf=0.97e7, sats=[(20, 12345, 250.0, 40.0, 2.0)],
                chans=[(20, 1000, 250, 8, 2, 0, 0.97e7)]),
    # one ring: the right carrier, twice that (half the compensation), none on a satellite that walks and none on one
    # at 0 Hz that does not; four grids, two of them compensated, three values of back
    "mixed": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=8, f_cf=F41,
                  sats=[(3, 100, -1000.0, 34.5, 0.1), (8, 1500, 1000.0, 34.5, 0.9), (22, 3210, 0.0, 34.5, 2.5)],
                  chans=[(3, 1000, 500, 40, 5, 0, F41), (3, 1000, 500, 40, 5, 0, 2 * F41), (8, 1000, 500, 40, 5, 0, 0.0),
                         (22, 1000, 500, 40, 5, 0, 0.0), (8, 1000, 500, 40, 5, 0, F41)]),
}


def nsamp(sc):
    return int(sc["f_sf"] * 1e-3)


def pair(gc, orc, sc, chan):
    """(device Channel, oracle channel) of one entry of a scenario's chans."""
    prn, hband, step, intg, ncoh, estep, f_cf = chan
    c = gc.Channel(prn, dtype=sc["dtype"], f_sf=sc["f_sf"], f_if=sc["f_if"], hband=hband, step=step, intg=intg, ncoh=ncoh,
                   estep=estep, f_cf=f_cf if f_cf else L1, cdop=f_cf != 0)
    o = ac.grid(orc.make_chan(prn, dtype=sc["dtype"], f_cf=c.f_cf, f_sf=sc["f_sf"], f_if=sc["f_if"]), hband, step, intg)
    assert o.nfreq == c.nfreq and np.array_equal(np.ctypeslib.as_array(o.freq)[:o.nfreq], c.freq)
    assert (o.f_if, o.foffset) == (c.f_if, c.foffset)
    return c, o


def sat_at(prn, at, f_sf, doppler, cn0, f_cf, phase, into=0.5):
    """A satellite whose code periods start `into` samples before stream sample `at` (and every period of its own from
    there); its code runs at crate*(1 + doppler/f_cf) (synth.make_if)."""
    crate = 1.023e6
    rate = crate * (1.0 + doppler / f_cf)
    cph = (into * crate / f_sf - rate * at / f_sf) % 1023.0
    return dict(prn=prn, doppler=float(doppler), codephase=float(cph), cn0=float(cn0), phase=float(phase))


def span_len(orc_pairs, sc):
    n, intg = nsamp(sc), sc["chans"][0][3]
    assert all(ch[3] == intg for ch in sc["chans"])
    backs = [chan_shifts(o, ch[4], ch[6])[1] for (_, o), ch in zip(orc_pairs, sc["chans"])]
    return (intg + 1) * n + max(backs), backs


def make_span(gc, synth, sc, pairs, seed=None, cn0=None):
    """The scenario's span W.  seed / cn0 replace the scenario's seed and the C/N0 of its satellites (the C/N0 search
    of tests/test_acq_slip_host.py)."""
    n, ncoh = nsamp(sc), sc["chans"][0][4]
    N, backs = span_len(pairs, sc)
    origin = N - backs[0] - (sc["chans"][0][3] + 1) * n         # b0 of the first channel
    sats = []
    for t in sc["sats"]:
        prn, lag, dop, c, ph = t[:5]
        at = origin + lag + (ncoh // 2) * n
        a = sat_at(prn, at, sc["f_sf"], dop, c if cn0 is None else cn0, sc["f_cf"], ph)
        if len(t) > 5:
            # the data bit flips where the satellite's period t[5] starts: a second copy, carrier turned by pi, takes over
            b = dict(a)
            period = n / (1.0 + dop / sc["f_cf"])
            a["t_off"] = b["t_on"] = (at - 0.5 + (t[5] - ncoh // 2) * period) / sc["f_sf"]
            b["phase"] = a["phase"] + math.pi
            sats.append(b)
        sats.append(a)
    codes = {s["prn"]: gc.gencode(s["prn"], gc.CTYPE_L1CA) for s in sats}
    return synth.make_if(codes, N, f_sf=sc["f_sf"], f_if=sc["f_if"], dtype=sc["dtype"], sats=sats,
                         seed=sc["seed"] if seed is None else seed, f_cf=sc["f_cf"])


def restate(orc, pairs, chans, ring_buf, ringlen, wrpos):
    jobs = [lambda o=o, ch=ch: slip_acq(orc, o, ring_buf, ringlen, wrpos, ch[4], ch[6], ch[5])
            for (_, o), ch in zip(pairs, chans)]
    return ac.run_oracles(jobs)


_cache = {}


def scenario(gc, orc, synth, name):
    """(span W, [(Channel, oracle channel)], [restated result]) of a scenario, the ring being W itself and the search
    ending at its last sample: computed once per process."""
    if name not in _cache:
        sc = SCEN[name]
        pairs = [pair(gc, orc, sc, ch) for ch in sc["chans"]]
        W = make_span(gc, synth, sc, pairs)
        _cache[name] = (W, pairs, restate(orc, pairs, sc["chans"], W, len(W), len(W)))
    return _cache[name]
