"""Carrier frequency refinement of acquired channels (gnsscorr_acq_set_refine): a restatement of its
semantics on the host, and the scenarios of tests/test_acq_fine_host.py (accuracy and decision margins, on the
restatement alone) and tests/test_gpu_acq_fine.py (which runs them on the device).  Helpers; not a conftest.

The restatement (`fine_freq`) for a channel with result `res` of a search, n = nsamp, K = 256:
  1. the nref*n ring samples from res.buffloc on;
  2. one literal mixcarr() call over them at res.acqfreq, phase 0 at the first (orc_mixcarr_seq: integers I, Q);
  3. the oracle's resampled code rc[k], k < n (orc_rescode_seq with the channel's ci and no offset);
  4. P_m = sum_k rc[k] (I + iQ)[m n + k] in numpy int64;
  5. S_m = P_m^2 in int64 (I^2 - Q^2, 2 I Q), converted to fp64; |S_m| = I^2 + Q^2 likewise;
  6. Z[q] = sum_m S_m exp(+2 pi i ((q m) mod K)/K) for q = -K/2 .. K/2-1 in fp64, q* the first largest |Z|^2;
  7. finefreq = acqfreq + q*/(2 K ctime), quality = |Z[q*]|^2 / (sum_m |S_m|)^2.
A channel that is not acquired or has nref = 0 gets rule 8: finefreq = acqfreq, zeros.

Satellites sit off the bin centres of the grids that search them: -90, -37, +13 and +90 Hz off a 200 Hz grid's bins, and
+20 Hz off a 50 Hz grid's bin for the channel that integrates ten periods with bit-edge hypotheses.
"""
import math

import numpy as np

import acq_cases as ac
import acq_coh_cases as cc
import acq_edge_cases as ec
from acq_cases import push_wrapping, ring_order, sat_at, span, wrap_points  # noqa: F401  (shared by import)

K = 256                     # GNSSCORR_FINE_BINS
MAXCOH = 20                 # GNSSCORR_MAXCOH
GAP = 1e-9                  # relative gap the winning |Z|^2 needs over every other q for q* to be an exact comparison


def step(ctime):
    """One step of the estimator's grid, Hz."""
    return 1.0 / (2.0 * K * ctime)


def rule8(res):
    return dict(finefreq=res["acqfreq"], quality=0.0, q=0, nref=0, prompt=np.zeros((MAXCOH, 2), np.int64), gap=1.0)


def fine_freq(orc, o, ring_buf, ringlen, res, nref):
    """Rules 1-7 (8 for a channel without refinement) for oracle channel `o` and its search result `res` (a dict with
    flagacq, buffloc, acqfreq).  Returns dict(finefreq, quality, q, nref, prompt = (MAXCOH, 2) int64 with zero rows
    beyond nref, gap = relative gap between the largest |Z|^2 and the next largest over all other q)."""
    if not res["flagacq"] or nref == 0:
        return rule8(res)
    n = o.nsamp
    cnt = nref * n
    idx = (int(res["buffloc"]) + np.arange(cnt, dtype=np.int64)) % ringlen
    win = np.ascontiguousarray(ring_buf[idx])
    I = np.zeros(cnt + 64, np.int16)
    Q = np.zeros(cnt + 64, np.int16)
    orc.lib().orc_mixcarr_seq(win.ctypes.data, o.dtype, o.ti, cnt, float(res["acqfreq"]), 0.0, I.ctypes.data,
                              Q.ctypes.data)
    code = np.ascontiguousarray(np.ctypeslib.as_array(o.code)[:o.clen])
    rc = np.zeros(n, np.int16)
    orc.lib().orc_rescode_seq(code.ctypes.data, o.clen, 0.0, 0, o.ci, n, rc.ctypes.data)
    rc = rc.astype(np.int64)
    PI = I[:cnt].astype(np.int64).reshape(nref, n) @ rc
    PQ = Q[:cnt].astype(np.int64).reshape(nref, n) @ rc
    Sr = (PI * PI - PQ * PQ).astype(np.float64)
    Si = (2 * PI * PQ).astype(np.float64)
    Sa = (PI * PI + PQ * PQ).astype(np.float64)
    q = np.arange(-K // 2, K // 2, dtype=np.int64)
    arg = 2.0 * ((q[:, None] * np.arange(nref, dtype=np.int64)[None, :]) % K).astype(np.float64) / K
    cs, sn = np.cos(np.pi * arg), np.sin(np.pi * arg)
    zr = (Sr[None, :] * cs - Si[None, :] * sn).sum(axis=1)
    zi = (Sr[None, :] * sn + Si[None, :] * cs).sum(axis=1)
    Z2 = zr * zr + zi * zi
    k = int(np.argmax(Z2))                              # the first of equal maxima: the lowest q
    others = np.delete(Z2, k)
    den = float(Sa.sum())
    prompt = np.zeros((MAXCOH, 2), np.int64)
    prompt[:nref, 0], prompt[:nref, 1] = PI, PQ
    return dict(finefreq=float(res["acqfreq"]) + float(q[k]) / (2.0 * K * o.ctime),
                quality=float(Z2[k]) / (den * den) if den > 0 else 0.0, q=int(q[k]), nref=nref, prompt=prompt,
                gap=float((Z2[k] - others.max()) / Z2[k]) if Z2[k] > 0 else 0.0)


# ---- scenarios ------------------------------------------------------------------------------------------------------
# The format of tests/acq_edge_cases.py: sats (prn, lag, doppler Hz, C/N0 dB-Hz, carrier phase[, sample from which the
# data bit is flipped]); chans (prn, hband, step, intg, ncoh, estep).  Dopplers are a bin centre plus the offset named.
N4, N2, N26 = 4092, 2048, 26000
SCEN = {
    # 4.092 Msps IQ, 200 Hz grids of 15 bins: the four offsets, a data bit flipped inside two of the refine spans (at a
    # period boundary of the satellite and in mid-period), an absent PRN
    "iq4": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=31,
                sats=[(3, 100, 600.0 - 90.0, 46.0, 0.1), (8, 1500, -1000.0 - 37.0, 45.0, 0.9, 1500 + 3 * N4),
                      (14, 3000, 400.0 + 13.0, 44.0, 1.7), (22, 4000, -200.0 + 90.0, 47.0, 2.5, 4000 + 6 * N4 + 2046)],
                chans=[(3, 1400, 200, 10, 1, 0), (8, 1400, 200, 10, 1, 0), (14, 1400, 200, 10, 1, 0),
                       (22, 1400, 200, 10, 1, 0), (5, 1400, 200, 10, 1, 0)]),
    # real samples at an IF of a quarter of the sample rate
    "real4": dict(f_sf=4.092e6, f_if=1.023e6, dtype=1, seed=32,
                  sats=[(13, 999, -400.0 + 90.0, 47.0, 1.0), (20, 2222, 200.0 - 37.0, 46.0, 0.4, 2222 + 4 * N4)],
                  chans=[(13, 1000, 200, 10, 1, 0), (20, 1000, 200, 10, 1, 0)]),
    # 2.048 Msps IQ: two samples per chip, the smallest period
    "iq2": dict(f_sf=2.048e6, f_if=0.0, dtype=2, seed=33,
                sats=[(6, 1000, 800.0 + 13.0, 47.0, 0.6), (17, 333, -600.0 - 90.0, 46.0, 2.2, 333 + 2 * N2)],
                chans=[(6, 1000, 200, 10, 1, 0), (17, 1000, 200, 10, 1, 0)]),
    # one group of ten periods with every bit-edge hypothesis on a 50 Hz grid, the satellite +20 Hz off a bin and its
    # data flipped on its fourth period boundary
    # (seed 34 left one of the nine rows with tied hypotheses, more than acq_edge_cases.check_margins allows; 35 does not)
    "coh": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=35,
                sats=[(9, 3210, 150.0 + 20.0, 43.0, 0.2, 3210 + 4 * N4)],
                chans=[(9, 200, 50, 10, 10, 1)]),
    # 26 Msps IQ, periods of 26000 samples: the 65536-point search and the largest prompt sums; a three-bin grid
    "m26": dict(f_sf=26e6, f_if=0.0, dtype=2, seed=35, sats=[(25, 12345, 200.0 - 37.0, 50.0, 2.0)],
                chans=[(25, 200, 200, 4, 1, 0)]),
}
SMALL = ("iq4", "real4", "iq2")


def nrefs(sc):
    """The nref values a scenario is run with: 2 and intg."""
    return (2, sc["chans"][0][3])


def f_true(sc, prn):
    """The carrier frequency of the scenario's satellite `prn` as the search sees it (None: absent)."""
    for t in sc["sats"]:
        if t[0] == prn:
            return sc["f_if"] + t[2]
    return None


_cache = {}


def scenario(gc, orc, synth, name):
    """(span W, [(Channel, oracle channel)], [restated search result]) of a scenario, the ring being W itself and the
    search ending at its last sample (acq_edge_cases.edge_acq: the restated search with groups and hypotheses, the
    reference's for ncoh = 1): computed once per process."""
    if name not in _cache:
        sc = SCEN[name]
        W = ec.make_span(gc, synth, sc)
        pairs = [ec.pair(gc, orc, sc, ch) for ch in sc["chans"]]
        _cache[name] = (W, pairs, ec.restate(orc, pairs, W, len(W), len(W)))
    return _cache[name]


# The hand-over test's signal: the search span and 205 periods to track behind it, two satellites off their bin centres
# and an absent PRN, channels on the 15-bin 200 Hz grid of `iq4`.  The search ends at period 11 of the stream.
HO_PRNS, HO_DOP, HO_LAG = [3, 14, 5], [600.0 - 90.0, 400.0 + 13.0], [100, 3000]       # PRN 5 is absent
HO_PER, HO_WRPOS, HO_NREF = 216, 11 * N4, [10, 0, 10]


def handover_signal(gc, synth):
    if "ho" not in _cache:
        sats = [sat_at(p, lag, N4, 4.092e6, d, 47.0, phase=0.3 + i, mid=5) for i, (p, d, lag) in
                enumerate(zip(HO_PRNS, HO_DOP, HO_LAG))]
        codes = {s["prn"]: gc.gencode(s["prn"], gc.CTYPE_L1CA) for s in sats}
        _cache["ho"] = synth.make_if(codes, HO_PER * N4, f_sf=4.092e6, f_if=0.0, dtype=2, sats=sats, seed=51)
    return _cache["ho"]


def handover_pairs(gc, orc):
    """[(Channel, oracle channel)] of the hand-over test (fresh objects)."""
    sc = dict(dtype=2, f_sf=4.092e6, f_if=0.0)
    return [ec.pair(gc, orc, sc, (p, 1400, 200, 10, 1, 0)) for p in HO_PRNS]


def fine_all(orc, pairs, buf, ringlen, results, nref):
    """The restatement for every channel of `pairs` with its search result (nref: one value, or one per channel)."""
    nr = [nref] * len(pairs) if np.isscalar(nref) else list(nref)
    return [fine_freq(orc, o, buf, ringlen, r, k) for (_, o), r, k in zip(pairs, results, nr)]


# ---- spans for the accuracy tests of tests/test_acq_fine_host.py ------------------------------------------------------
def clean_cn0(amp, sigma, f_sf, dtype):
    """The C/N0 at which synth.make_if gives a satellite the amplitude `amp` on noise of `sigma`."""
    return 10.0 * math.log10((amp / sigma) ** 2 * f_sf / (2.0 if dtype == 2 else 4.0))


def lone_span(gc, synth, sc, sat, nper, cn0=None, seed=0, flip=None):
    """nper code periods of the scenario's front end with the satellite tuple `sat` alone: free of noise at amplitude
    40 (cn0 None; the generator's noise is scaled below the int8 rounding), or at `cn0` dB-Hz on the generator's noise
    with seed `seed`.  flip: the sample from which its data bit is inverted.  The satellite is exactly on its lag in
    the span's second period."""
    n = cc.nsamp(sc)
    sigma = 1e-6 if cn0 is None else 8.0
    prn, lag, dop, _, ph = sat[:5]
    a = sat_at(prn, lag, n, sc["f_sf"], dop, clean_cn0(40.0, sigma, sc["f_sf"], sc["dtype"]) if cn0 is None else cn0,
               phase=ph, mid=1)
    sats = [a]
    if flip is not None:
        b = dict(a)
        a["t_off"] = b["t_on"] = flip / sc["f_sf"]
        b["phase"] = a["phase"] + math.pi
        sats.append(b)
    codes = {prn: gc.gencode(prn, gc.CTYPE_L1CA)}
    return synth.make_if(codes, nper * n, f_sf=sc["f_sf"], f_if=sc["f_if"], dtype=sc["dtype"], sats=sats, seed=seed,
                         noise_sigma=sigma)


def nearest_bin(c, f):
    """The centre of the bin of Channel c's grid nearest to frequency f: what a search that finds the satellite
    returns as acqfreq."""
    return float(c.freq[int(np.argmin(np.abs(c.freq - f)))])
