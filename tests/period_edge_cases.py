"""Period lengths at which the kernels change shape: the scenarios of tests/test_period_edges_host.py (which shows on
the oracle alone that each is what it claims to be) and tests/test_gpu_period_edges.py (which runs them on the device).
Helpers; not a conftest.

Every length here is named by a line of the library:
  - acquisition (gnsscorr_acq.hip): nsamp <= 16384 takes the 32768-point transform, 16385 .. 32768 the 65536-point one
    (`c.nsamp > GC_LH`), above that the search is refused (`c.nsamp > GC_L`); at 16384 and 32768 the window of 2 nsamp
    samples is the whole transform, nothing is padded and every register slot of a power row is a live lag;
  - tracking (gc_trk_nseg, trk_ps_rounds; restated below as `nseg`, `rounds_per_seg`): a period is split over nseg
    workgroups of at most GC_MAXR = 24 rounds of 1024 samples, sized for nsamp + 100 samples;
  - the edge table (trk_expand_kernel): a unit gets one when its rounds touch 1 .. GC_EDGTAB = 704 chip edges and its
    n + 2 smax replica positions stay below 65535 (uint16 start samples).
A period of nsamp samples comes from a front end at f_sf = nsamp * 1e3 with the 1 ms codes; `pair` and `trk_scene` assert
that the library's and the oracle's channel set-up both arrive at that nsamp.
"""
import math
import os
import re

import numpy as np

import acq_cases as ac
import acq_coh_cases as cc
import acq_edge_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the tracking geometry, restated (gnsscorr_trk.hip: gc_trk_nseg; gnsscorr_ps.h: trk_ps_rounds, trk_ps_nit) ------
GC_MAXR, GC_PS_WLANES, GC_EDGTAB, NT_LIMIT = 24, 64, 704, 65535
NSAMP_MAX, ACQ_LH, ACQ_L = 262144, 16384, 32768


def groups(dtype, max_n):
    """16-byte sample groups a period of up to max_n samples can touch, wherever it starts in the ring."""
    return (15 + max_n * dtype + 15) // 16 + 1


def nit(dtype):
    """Groups per lane and round with the default GNSSCORR_TRK_NIT: 2, and 1 for real samples."""
    return 1 if dtype == 1 else 2


def rounds(dtype, nsamp):
    """Rounds (one wavefront's share: 64 * nit groups, 1024 samples) of a context whose longest period is nsamp."""
    return -(-groups(dtype, nsamp + 100) // (GC_PS_WLANES * nit(dtype)))


def nseg(dtype, nsamp):
    return -(-rounds(dtype, nsamp) // GC_MAXR)


def rounds_per_seg(dtype, nsamp):
    return -(-rounds(dtype, nsamp) // nseg(dtype, nsamp))


def first_nsamp(dtype, k):
    """The smallest nsamp with nseg >= k (nseg never falls as nsamp grows)."""
    lo, hi = 1, NSAMP_MAX + 1
    while lo < hi:
        mid = (lo + hi) // 2
        if nseg(dtype, mid) >= k:
            hi = mid
        else:
            lo = mid + 1
    return lo


def front_end(nsamp, dtype):
    """(f_sf, f_if) of the front end whose 1 ms code periods have nsamp samples: IQ at zero IF, real samples at a
    quarter of the sample rate."""
    f_sf = nsamp * 1e3
    return f_sf, (f_sf / 4.0 if dtype == 1 else 0.0)


def check_nsamp(c, o, nsamp):
    assert c.nsamp == o.nsamp == nsamp, (c.nsamp, o.nsamp, nsamp)
    assert c.nsampchip == o.nsampchip == nsamp // c.clen


# ---- the int32 bound ------------------------------------------------------------------------------------------------
def header_lut():
    """(cos32, sin32) as gnsscorr_lut.h states them: the table every kernel of the library wipes carriers off with."""
    txt = open(os.path.join(ROOT, "erlangnetwork-gnsslib-sdr_amd", "csrc", "gnsscorr_lut.h")).read()
    out = []
    for name in ("gcCos32", "gcSin32"):
        m = re.search(name + r"\[32\]\s*=\s*\{([^}]*)\}", txt)
        v = np.array([int(x) for x in m.group(1).split(",")], np.int64)
        assert v.shape == (32,)
        out.append(v)
    return out


def device_lut(gc):
    """The same table read off the device: mixcarr() of the library over 32 unit samples half a cell into each entry."""
    one = np.ones(32, np.int8)
    I, Q = np.zeros(32, np.int16), np.zeros(32, np.int16)
    gc.lib().mixcarr(one.ctypes.data, 1, 1.0, 32, 1.0 / 32.0, 2.0 * math.pi * 0.5 / 32.0, I.ctypes.data, Q.ctypes.data)
    return I.astype(np.int64), Q.astype(np.int64)


def accumulator_bound(cos32, sin32):
    """The largest |sum| a tap can reach: nsamp + 100 samples (the longest period tracked), each an IQ pair of int8
    extremes wiped off to |cos d.x - sin d.y| <= 128 (|cos| + |sin|), every one of the replica's sign."""
    return (NSAMP_MAX + 100) * 128 * int(np.max(np.abs(cos32) + np.abs(sin32)))


# ---- tracking scenes ------------------------------------------------------------------------------------------------
TAPS5, TAPS33 = (2, 3, 3), (16, 4, 4)       # (corrn, corrd, corrp): 5 taps out to 6 samples; 33 out to 64
NPER = 6                                    # two batches of three periods
_cache = {}


def trk_lengths(dtype):
    """[(name, nsamp)] of the batched tracking cases: the lengths on either side of every boundary."""
    two, three = first_nsamp(dtype, 2), first_nsamp(dtype, 3)
    return [("one_sample_per_chip", 1023), ("last_nseg1", two - 1), ("first_nseg2", two), ("acq_limit", ACQ_L),
            ("last_nseg2", three - 1), ("first_nseg3", three), ("table_65000", 65000), ("no_table_65535", 65535),
            ("no_table_65536", 65536), ("nseg6_131072", 131072), ("nseg11_262144", NSAMP_MAX)]


def first_period(c, st):
    """currnsamp of the first period from state st (ref src/sdrtrk.c:31)."""
    return int((c.clen - st["remcode"]) / (st["codefreq"] / c.f_sf))


def tail_edge(code):
    """The code's last chip differs from its first: a chip edge where the period ends, at replica position n + smax."""
    return int(code[-1]) != int(code[0])


def ring_samples(nsamp, nch, dtype, nper=NPER, buffloc0=5):
    """A ring that holds nper periods of every channel behind _setup's start positions and one more period behind them
    (the reference tracks a period once wrpos - nsamp has passed its first sample), on the ring's 16-byte granule."""
    return ec.granule(buffloc0 + 1000 * nch + (nper + 1) * (nsamp + 2), dtype)


def trk_scene(gc, orc, key, dtype, nsamp, prns=(1, 7, 13, 32), taps=TAPS5, seed=None, ftype=1, tweak=None, nper=NPER):
    """Samples, channels, start states (tests/test_gpu_tracking.py::_setup's mix: a channel fresh out of acquisition,
    one with an integer code phase, the others mid-track, start positions unaligned) and the oracle's nper periods of
    them: dict(data, nsamples, chans, states, oII, oQQ, ons, ofin, ...).  tweak(chans, states, ochs) edits them before
    the oracle runs.  Computed once per process under `key`."""
    if key in _cache:
        return _cache[key]
    from test_gpu_tracking import _oracle_run, _setup
    fs, f_if = front_end(nsamp, dtype)
    nsamples = ring_samples(nsamp, len(prns), dtype, nper)
    seed = seed if seed is not None else 7000 + nsamp % 1000 + dtype
    data, chans, states, ochs = _setup(gc, orc, None, dtype, f_if, *taps, prns=list(prns), nsamples=nsamples, seed=seed,
                                       buffloc0=5, f_sf=fs, ftype=ftype, apply=False)
    for c, o in zip(chans, ochs):
        check_nsamp(c, o, nsamp)
    if tweak is not None:
        tweak(chans, states, ochs)
    for c, st in zip(chans, states):            # (the oracle's scratch, like the reference's, is nsamp + 100 samples)
        assert 0 < first_period(c, st) <= nsamp + 100, (c.prn, first_period(c, st))
    oII, oQQ, ons, ofin = _oracle_run(orc, ochs, states, data, nsamples, nsamples, nper)
    assert ons.max() <= nsamp + 100
    sc = dict(key=key, dtype=dtype, nsamp=nsamp, ftype=ftype, data=data, nsamples=nsamples, chans=chans, states=states,
              oII=oII, oQQ=oQQ, ons=ons, ofin=ofin, smax=int(chans[0].corrp[-1]), ntap=chans[0].ntap)
    _cache[key] = sc
    return sc


def length_scene(gc, orc, dtype, nsamp, ftype=1, prns=None):
    """The plain scene of one length: four channels."""
    if prns is None:
        prns = (1, 7, 13, 32)
    return trk_scene(gc, orc, ("len", dtype, nsamp, ftype, tuple(prns)), dtype, nsamp, prns=prns, ftype=ftype)


def nt(sc):
    """n + 2 smax of every (channel, period): the replica positions the unit's edge table would have to address."""
    return sc["ons"] + 2 * sc["smax"]


# PRNs 7 and 32 of _setup's mix end on a chip other than their first (asserted by the host tests): with a period of
# 65530 samples or more their closing edge starts at a replica position n + smax > 65535, which a uint16 cannot hold.
STRADDLE_NSAMP = 65532


def straddle_scene(gc, orc, dtype):
    """One channel set at 65532 samples in which the edge-table condition changes inside a channel's batch:
    channel 2 starts 0.2 chips into its code at the nominal rate -- a first period of 65519 samples (65531 replica
    positions: a table) and periods of 65531 / 65532 after it (65543 / 65544: none, the closing edge beyond 65535);
    channel 3 runs its code 148 Hz fast, periods of 65522 and 65523 samples in turn: 65534 and 65535 replica positions,
    the two sides of `u.nt < 65535` itself."""
    def tweak(chans, states, ochs):
        states[2].update(codefreq=chans[2].crate, remcode=0.2)
        states[3].update(codefreq=chans[3].crate * STRADDLE_NSAMP / (STRADDLE_NSAMP - 9.5))
    return trk_scene(gc, orc, ("straddle", dtype), dtype, STRADDLE_NSAMP, prns=(1, 13, 7, 32), tweak=tweak)


CODES_NSAMP = 16368


def alternating_code():
    c = np.ones(1023, np.int16)
    c[1::2] = -1
    return c


def codes_scene(gc, orc, dtype):
    """Three channels at 16368 samples whose codes go in through gnsscorr_chan_t.code: one that alternates every chip
    (1022 edges per period: more than the table's 704, no table), a constant one (no edge: no table) and PRN 13 (a
    table): one launch holds units with and without a table."""
    def tweak(chans, states, ochs):
        for i, code in ((0, alternating_code()), (1, np.ones(1023, np.int16))):
            chans[i].code = code.copy()
            np.ctypeslib.as_array(ochs[i].code)[:] = code
    return trk_scene(gc, orc, ("codes", dtype), dtype, CODES_NSAMP, prns=(1, 7, 13), tweak=tweak)


def code_edges(code):
    """Chip edges of one code period, the closing one included."""
    code = np.asarray(code)
    return int(np.count_nonzero(code != np.roll(code, 1)))


def full_scale_scene(gc, orc, dtype):
    """262144 samples per period, 33 taps out to 64 samples, every sample an int8 extreme (the arrangement of
    tests/test_gpu_tap_sets.py::test_full_scale_samples_33_taps_26msps): the in-phase rail is PRN 1's code at the
    nominal rate with the opposite sign, -128 under a +1 chip; the IQ ring's other rail carries the code itself.
    Channel 0 tracks PRN 1 on a carrier of 0 Hz at phase 0 (I = 32 d.x); channel 1 the same code at a constant phase
    of 4.5 cells, cos = sin = 23: I = 23 (d.x - d.y), every sample -255 times the chip -- 0.99 of the bound
    `accumulator_bound` states.  Channel 2 is mid-track."""
    key = ("full", dtype)
    if key in _cache:
        return _cache[key]
    from test_gpu_tracking import _oracle_run
    nsamp = NSAMP_MAX
    f_sf, f_if = nsamp * 1e3, 0.0
    prns = (1, 1, 19)
    nsamples = ring_samples(nsamp, len(prns), dtype)
    rng = np.random.default_rng(262 + dtype)
    code, crate = gc.gencode(1, gc.CTYPE_L1CA)
    k = np.arange(nsamples)
    chip = np.floor(k * (crate / f_sf)).astype(np.int64) % 1023
    rail = np.where(code[chip] > 0, np.int8(-128), np.int8(127))
    rail[rng.random(nsamples) < 0.01] = -127
    if dtype == 2:
        other = np.where(code[chip] > 0, np.int8(127), np.int8(-128))
        other[rng.random(nsamples) < 0.01] = -127
        data = np.ascontiguousarray(np.stack([rail, other], axis=1))
    else:
        data = rail
    chans = [gc.Channel(p, dtype=dtype, f_sf=f_sf, f_if=f_if, corrn=TAPS33[0], corrd=TAPS33[1], corrp=TAPS33[2])
             for p in prns]
    ochs = [orc.make_chan(p, dtype=dtype, f_sf=f_sf, f_if=f_if, corrn=TAPS33[0], corrd=TAPS33[1], corrp=TAPS33[2])
            for p in prns]
    for c, o in zip(chans, ochs):
        check_nsamp(c, o, nsamp)
    assert int(chans[0].corrp[-1]) == 64 and chans[0].ntap == 33
    states = [dict(carrfreq=0.0, codefreq=crate, remcode=0.0, remcarr=0.0, buffloc=0),
              dict(carrfreq=0.0, codefreq=crate, remcode=0.0, remcarr=2.0 * math.pi * 4.5 / 32.0, buffloc=0),
              dict(carrfreq=float(rng.uniform(-3000, 3000)), codefreq=crate + float(rng.uniform(-2, 2)),
                   remcode=float(rng.uniform(0, 1)), remcarr=float(rng.uniform(0, 6)), buffloc=3107)]
    oII, oQQ, ons, ofin = _oracle_run(orc, ochs, states, data, nsamples, nsamples, NPER)
    sc = dict(key=key, dtype=dtype, nsamp=nsamp, ftype=1, data=data, nsamples=nsamples, chans=chans, states=states,
              oII=oII, oQQ=oQQ, ons=ons, ofin=ofin, smax=64, ntap=33)
    _cache[key] = sc
    return sc


SHORT_NSAMP = 2048


def mixed_scenes(gc, orc, dtype, swapped):
    """(short, long): three 2048-sample channels on one ring and four 262144-sample channels on the other (ring 1 and
    ring 2, or swapped).  The context's segments are sized by the long period: ten of the eleven are empty for the short
    channels' units."""
    fs, fl = (2, 1) if swapped else (1, 2)
    return (length_scene(gc, orc, dtype, SHORT_NSAMP, ftype=fs, prns=(7, 13, 32)),
            length_scene(gc, orc, dtype, NSAMP_MAX, ftype=fl))


# ---- acquisition scenes ---------------------------------------------------------------------------------------------
# Three satellites and an absent PRN on a grid of five bins (hband 400, step 200), intg 2:
#   - one at lag 0, where checkacquisition()'s maxvd() seeds the second peak with element 0, the peak itself: a ratio of
#     exactly 1, never acquired (quirk Q3 of tests/test_gpu_acq_edges.py::test_lag_edges);
#   - one at lag nsamp - 1, the last live lag.  Element 0, one sample on, lies inside its exclusion window and seeds the
#     second peak all the same: at two samples per chip and more it holds most of the peak's power and the ratio stays
#     below ACQTH whatever the C/N0 or the noise; at one sample per chip (1023) it is a whole chip away and the channel is
#     acquired.  Lag, bin, cn0, peak ratio and power of both are still the oracle's, and what the device is held to;
#   - one at nsamp - 2 nsampchip on the outer bin, 37 Hz off its centre (for the refinement): its exclusion window ends
#     on element nsamp, i.e. wraps onto element 0, which is two chips away from the peak; acquired everywhere.
ACQ_GRID = (400, 200, 2)
ACQ_PRNS, ACQ_ABSENT = (3, 8, 14), 22
ACQ_DOP = (0.0, -200.0, 400.0 - 37.0)
ACQ_BIN = (2, 1, 4)
ACQ_SCEN = {
    # name: nsamp, dtype, C/N0 dB-Hz, span in periods (3: the search; 5: a search of two groups of two behind it; 8:
    # three periods to track behind a hand-over), seed
    "iq1023": dict(n=1023, dtype=2, cn0=50.0, periods=3, seed=1023),
    "iq16384": dict(n=16384, dtype=2, cn0=49.0, periods=3, seed=16384),
    "real16384": dict(n=16384, dtype=1, cn0=49.0, periods=3, seed=16385),
    "iq16385": dict(n=16385, dtype=2, cn0=49.0, periods=3, seed=16386),
    "iq32768": dict(n=32768, dtype=2, cn0=49.0, periods=8, seed=32768),
    "real32768": dict(n=32768, dtype=1, cn0=49.0, periods=3, seed=32889),
    # the spans of the coherent searches (ncoh 2, intg 4).  47 dB-Hz: a group of two periods lifts the peak 3 dB further
    # above the floor, to where a plain search has it at 50 dB-Hz -- the most at which the fp32 transforms' error, which
    # follows the peak, stays inside a bar stated in units of the floor (tests/test_gpu_acq_edges.py's module docstring)
    "coh16384": dict(n=16384, dtype=2, cn0=47.0, periods=5, seed=16387),
    "coh32768": dict(n=32768, dtype=2, cn0=47.0, periods=5, seed=32850),
}
PLAIN_SCEN = tuple(sorted(k for k in ACQ_SCEN if not k.startswith("coh")))
# C/N0: at 47 dB-Hz the one window that decides the acquired satellite left peak ratios of 3.1 to 5.0 (the largest of
# 32768 noise cells is 10 to 14 row means); 49 dB-Hz gives 5.1 and more.  Seeds: the first of seed0 + 40 k at which the
# noise leaves every peak on its lag -- at 32 samples per chip the neighbouring lag holds 0.94 of the peak's power --
# and every decision acq_cases.MARGIN from a tie (real32768: k = 3; coh32768: k = 2; the others k = 0).
COH_GRID = (400, 200, 4, 2)                 # hband, step, intg, ncoh
COH_SCEN = ("coh16384", "coh32768")


def acq_lags(n):
    nsc = n // 1023
    return (0, n - 1, n - 2 * nsc)


def acq_front(name):
    s = ACQ_SCEN[name]
    f_sf, f_if = front_end(s["n"], s["dtype"])
    return dict(dtype=s["dtype"], f_sf=f_sf, f_if=f_if)


def acq_span(gc, synth, name):
    """The scenario's samples: `periods` code periods, every satellite on its lag at the start of period 1, a thousandth
    of a chip into its code (acq_cases.sat_at: the code Doppler of 400 Hz moves it by a quarter of that per period)."""
    key = ("span", name)
    if key not in _cache:
        s = ACQ_SCEN[name]
        n, fe = s["n"], acq_front(name)
        sats = [ac.sat_at(p, lag, n, fe["f_sf"], d, s["cn0"], phase=0.4 + 1.1 * i, mid=1)
                for i, (p, lag, d) in enumerate(zip(ACQ_PRNS, acq_lags(n), ACQ_DOP))]
        codes = {x["prn"]: gc.gencode(x["prn"], gc.CTYPE_L1CA) for x in sats}
        _cache[key] = synth.make_if(codes, s["periods"] * n, f_sf=fe["f_sf"], f_if=fe["f_if"], dtype=fe["dtype"],
                                    sats=sats, seed=s["seed"])
    return _cache[key]


def acq_pairs(gc, orc, name, intg=ACQ_GRID[2], ncoh=1, ftype=1):
    """[(Channel, oracle channel)] of the scenario's three satellites and the absent PRN (fresh objects)."""
    fe, n = acq_front(name), ACQ_SCEN[name]["n"]
    out = []
    for p in ACQ_PRNS + (ACQ_ABSENT,):
        c, o = ec.pair(gc, orc, fe, (p, ACQ_GRID[0], ACQ_GRID[1], intg, ncoh, 0))
        c.ftype = ftype
        check_nsamp(c, o, n)
        assert c.nfreq == 5
        out.append((c, o))
    return out


def acq_scene(gc, orc, synth, name):
    """dict(W, n, wrpos = 3 n, pairs, wants = acq_cases.oracle_acq of every channel over W): once per process."""
    key = ("acq", name)
    if key not in _cache:
        W, n = acq_span(gc, synth, name), ACQ_SCEN[name]["n"]
        pairs = acq_pairs(gc, orc, name)
        wrpos = (ACQ_GRID[2] + 1) * n
        wants = ac.run_oracles([lambda o=o: ac.oracle_acq(orc, o, W, len(W), wrpos) for _, o in pairs])
        _cache[key] = dict(name=name, W=W, n=n, wrpos=wrpos, pairs=pairs, wants=wants, dtype=ACQ_SCEN[name]["dtype"])
    return _cache[key]


def coh_scene(gc, orc, synth, name):
    """The same span searched with ncoh 2, intg 4 from its first sample on (wrpos = 5 n), against
    acq_coh_cases.coh_acq."""
    key = ("coh", name)
    if key not in _cache:
        W, n = acq_span(gc, synth, name), ACQ_SCEN[name]["n"]
        pairs = acq_pairs(gc, orc, name, intg=COH_GRID[2], ncoh=COH_GRID[3])
        wrpos = (COH_GRID[2] + 1) * n
        assert wrpos <= len(W)
        wants = ac.run_oracles([lambda o=o: cc.coh_acq(orc, o, W, len(W), wrpos, COH_GRID[3]) for _, o in pairs])
        _cache[key] = dict(name=name, W=W, n=n, wrpos=wrpos, pairs=pairs, wants=wants, dtype=ACQ_SCEN[name]["dtype"])
    return _cache[key]


def power_ratio_full(Pdev, Pref, codei, nsampchip):
    """max over every bin and lag of |P_dev - P_ref| / (the row's mean of P_ref outside codei's exclusion window)."""
    assert Pdev.shape == Pref.shape
    mask = ac.exclusion_mask(Pref.shape[1], codei, nsampchip)
    mean = Pref[:, mask].mean(axis=1)
    assert np.all(mean > 0)
    return float(np.max(np.abs(Pdev - Pref) / mean[:, None]))


def check_intended(sc, min_ratio=1.5 * 3.0):
    """The oracle finds every satellite at its lag and bin: the acquired ones with a peak ratio of at least 1.5 ACQTH,
    the two that element 0 keeps from being acquired (above) with the ratio that says so; the absent PRN fails."""
    n = sc["n"]
    for (c, _), w, lag, b in zip(sc["pairs"][:3], sc["wants"][:3], acq_lags(n), ACQ_BIN):
        assert (w["acqcodei"], w["freqi"]) == (lag, b), (sc["name"], c.prn, w["acqcodei"], w["freqi"])
        assert w["acqfreq"] == c.freq[b]
        assert int(np.argmax(w["P"][b])) == lag and w["P"][b, lag] == w["P"].max()
        if lag == 0:
            assert w["peakr"] == 1.0 and not w["flagacq"], (sc["name"], c.prn, w["peakr"])
        elif lag == n - 1 and n >= 2046:
            assert w["peakr"] == w["P"][b, lag] / w["P"][b, 0] < 2.0 and not w["flagacq"], (sc["name"], c.prn, w["peakr"])
        else:
            assert w["flagacq"] and w["peakr"] >= min_ratio, (sc["name"], c.prn, w["peakr"])
            assert w["buffloc"] == w["b0"] + lag
        if not w["flagacq"]:
            assert w["iters"] == c.intg and w["buffloc"] == w["b0"] + c.intg * n
    assert not sc["wants"][3]["flagacq"] and sc["wants"][3]["peakr"] < 3.0
    # the window of the satellite near the end wraps, by exactly one element; the last lag's by 2 nsampchip
    nsc = n // 1023
    m = ac.exclusion_mask(n, acq_lags(n)[2], nsc)
    assert not m[0] and m[1] and not m[n - 1] and int((~m).sum()) == 4 * nsc + 1
