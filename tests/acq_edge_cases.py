"""Bit-edge hypotheses for coherent groups (gnsscorr_acq_set_bitedge): a restatement of their
semantics on the host, and the scenarios of tests/test_acq_edge_host.py (which shows on the restatement alone that
each is decided with room), tests/test_gpu_acq_bitedge.py (which runs them on the device, the ring being the span) and
tests/test_gpu_acq_bitedge_positions.py (which runs them elsewhere in a stream and a ring: `position`, `moved_stream`,
and `rule6`, the documented meaning of an edge held against where the bit was flipped).  Helpers; not a conftest.

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
    # edge steps that do not divide ncoh: hypotheses {0,3,6,9}, {0,4,8}, {0,9} of 10 and {0,4} of 5 (H = ceil(ncoh /
    # estep) = 4, 3, 2, 2), each acquired channel's edge on the *last* of them, the one a floor would drop; an absent PRN
    "odd": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=13,
                sats=[(22, 2345, -150.0, 42.0, 2.6, _flip(2345, 9)), (7, 3000, 100.0, 42.0, 0.7, _flip(3000, 8)),
                      (9, 3210, 100.0, 42.0, 0.2, _flip(3210, 4))],
                chans=[(22, 200, 50, 10, 10, 3), (7, 200, 50, 10, 10, 4), (22, 200, 50, 10, 10, 9),
                       (9, 400, 100, 10, 5, 4), (5, 200, 50, 10, 10, 3)]),
    # the smallest H: ncoh 2, estep 1, five groups of two slots.  The 40 dB-Hz satellite passes at group 3 with rows
    # of hypotheses 0, 0, 1 summed; the 46 dB-Hz one at group 1; an absent PRN runs all five
    "two": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=12,
                sats=[(7, 2345, 250.0, 40.0, 0.7, _flip(2345, 5)), (11, 3000, -250.0, 46.0, 1.9, _flip(3000, 1))],
                chans=[(7, 500, 250, 10, 2, 1), (11, 500, 250, 10, 2, 1), (5, 500, 250, 10, 2, 1)]),
    # the largest: ncoh 20 = GNSSCORR_MAXCOH with every hypothesis, H = maxslot = 20, a carrier walk of 21 periods;
    # an edge at 19 (all windows but one negated) and one at 10
    "twenty": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=13,
                   sats=[(9, 3210, 25.0, 40.0, 0.2, _flip(3210, 19)), (14, 2345, -50.0, 40.0, 1.1, _flip(2345, 10))],
                   chans=[(9, 100, 25, 20, 20, 1), (14, 100, 25, 20, 20, 1), (5, 100, 25, 20, 20, 1)]),
    # a span of 13 periods searched twice by intg 10 channels, at its periods 0..10 and 2..12: the edges move with the
    # search (3 -> 1, outside -> 9, none, 1 -> before the span).  The satellites run through both searches
    "moved": dict(f_sf=4.092e6, f_if=0.0, dtype=2, seed=28, periods=13,
                  sats=[(22, 2345, -150.0, 42.0, 2.6, _flip(2345, 3)), (7, 3000, 100.0, 42.0, 0.7, _flip(3000, 11)),
                        (11, 3210, -100.0, 42.0, 1.9), (9, 2345, 50.0, 42.0, 0.2, _flip(2345, 1))],
                  chans=[(22, 200, 50, 10, 10, 1), (7, 200, 50, 10, 10, 1), (11, 200, 50, 10, 10, 1),
                         (9, 200, 50, 10, 10, 1), (5, 200, 50, 10, 10, 1)]),
}


def pair(gc, orc, sc, chan):
    """(device Channel, oracle channel) of one entry of a scenario's chans."""
    c, o = cc.pair(gc, orc, sc, chan[:5])
    c.estep = chan[5]
    return c, o


def make_span(gc, synth, sc):
    """The scenario's span: acq_coh_cases.make_span, (max intg + 1)*n samples, or sc["periods"] code periods where the
    scenario names a length (sized as a search of periods - 1 windows would size it: the satellites are on their lags
    in its middle and run through all of it)."""
    if "periods" in sc:
        sc = dict(sc, chans=list(sc["chans"]) + [(0, 0, 1, sc["periods"] - 1, 1, 0)])
    return cc.make_span(gc, synth, sc)


def restate(orc, pairs, ring_buf, ringlen, wrpos):
    """The restated search of every (Channel, oracle channel) of `pairs` that ends at write position wrpos of a ring."""
    return ac.run_oracles([lambda c=c, o=o: edge_acq(orc, o, ring_buf, ringlen, wrpos, c.ncoh, c.estep)
                           for c, o in pairs])


_cache = {}


def scenario(gc, orc, synth, name):
    """(span W, [(Channel, oracle channel)], [restated result]) of a scenario, the ring being W itself and the search
    ending at its last sample: computed once per process."""
    if name not in _cache:
        sc = SCEN[name]
        W = make_span(gc, synth, sc)
        pairs = [pair(gc, orc, sc, ch) for ch in sc["chans"]]
        _cache[name] = (W, pairs, restate(orc, pairs, W, len(W), len(W)))
    return _cache[name]


# ---- positions: the same span elsewhere in a stream and in a ring ---------------------------------------------------
def granule(nsamples, dtype):
    """nsamples rounded up to the ring's 16-byte granule."""
    g = 16 // dtype
    return -(-nsamples // g) * g


def placed(W, dtype, ringlen, b0, seed=77):
    """The span W from sample b0 of a stream on, noise in front of it: (stream, ringlen, wrpos = b0 + len(W)).  After
    the stream went in, the ring's last slot holds span sample ringlen - 1 - b0 when b0 < ringlen."""
    assert ringlen >= len(W) and b0 >= 0
    return np.concatenate([ac.noise(b0, dtype, seed), W]), ringlen, b0 + len(W)


def wrap_layouts(n, intg, dtype):
    """name -> (ringlen, b0) for a span of (intg+1)*n samples: rings of 13 periods that end 3.5 and 7.5 periods into
    the span, and a ring of exactly the span (rounded up to the granule) in front of which an odd number of samples
    went by (2 1/3 periods: the ring's end falls two thirds into the span's window intg - 2)."""
    r13, rx = granule((intg + 3) * n, dtype), granule((intg + 1) * n, dtype)
    return {"3.5": (r13, r13 - (3 * n + n // 2)), "7.5": (r13, r13 - (7 * n + n // 2)),
            "exact": (rx, (2 * n + n // 3) | 1)}


POSITIONS = [("groups5", "3.5"), ("groups5", "7.5"), ("groups5", "exact"), ("odd", "3.5"), ("real", "odd"),
             ("groups5", "2^32")]


def position(gc, orc, synth, name, layout):
    """Scenario `name` away from the origin: dict(stream, buf = the ring as the device holds it, ringlen, wrpos, b0 =
    where the span begins in the stream, K = ring lengths to commit after pushing the stream (the 2^32 layout only),
    wants = the restatement over buf), computed once per process.
    Layouts: those of wrap_layouts; "odd": a ring of intg + 3 periods that ends an odd number of samples, 2.5 periods
    and one, into the span; "2^32": the ring of tests/test_gpu_positions.py, 2^32 between the span's periods 3 and 4."""
    key = (name, layout)
    if key not in _cache:
        sc = SCEN[name]
        W, pairs, _ = scenario(gc, orc, synth, name)
        n, dtype = cc.nsamp(sc), sc["dtype"]
        intg = len(W) // n - 1
        K = None
        if layout == "2^32":
            from test_gpu_positions import high_layout
            T = 1 << 32
            ringlen, K = high_layout(T, (intg + 2) * n, 16 // dtype, (intg - 3) * n, (intg - 2) * n)
            wrpos = (K + 1) * ringlen
            b0 = wrpos - len(W)
            assert b0 + 2 * n < T < b0 + 5 * n
            buf = stream = np.concatenate([ac.noise(ringlen - len(W), dtype, 78), W])
        else:
            if layout == "odd":
                ringlen = granule((intg + 3) * n, dtype)
                b0 = ringlen - (2 * n + n // 2 + 1)
                assert b0 % 2 == 1
            else:
                ringlen, b0 = wrap_layouts(n, intg, dtype)[layout]
            stream, ringlen, wrpos = placed(W, dtype, ringlen, b0)
            assert b0 < ringlen < wrpos             # the ring's end lies inside the span
            buf = ac.ring_order(stream, ringlen, wrpos)
        _cache[key] = dict(stream=stream, buf=buf, ringlen=ringlen, wrpos=wrpos, b0=b0, K=K,
                           wants=restate(orc, pairs, buf, ringlen, wrpos))
    return _cache[key]


MOVED_B0 = 5 * N4 + 123       # where the span of `moved` begins in its stream


def moved_origin(gc, orc, synth):
    """`moved` restated on its span alone: [results of the search that ends at period 11, at period 13 (the
    scenario's own)], computed once per process."""
    if "moved@11" not in _cache:
        W, pairs, _ = scenario(gc, orc, synth, "moved")
        _cache["moved@11"] = restate(orc, pairs, W, len(W), 11 * N4)
    return [_cache["moved@11"], scenario(gc, orc, synth, "moved")[2]]


def moved_stream(gc, orc, synth):
    """(stream = noise(MOVED_B0) ++ W, ringlen: the ring holds it whole, the two write positions searched)."""
    W = scenario(gc, orc, synth, "moved")[0]
    stream, ringlen, wrpos = placed(W, 2, granule(MOVED_B0 + len(W), 2), MOVED_B0, seed=79)
    return stream, ringlen, [MOVED_B0 + 11 * N4, wrpos]


def same_search(want, ref, b0):
    """The restatement at another position (span from sample b0 on) against the one at the origin: the same samples,
    hence the same search -- every group's figures, the chosen hypotheses, the edge; positions moved by b0."""
    assert want["b0"] == ref["b0"] + b0, (want["b0"], ref["b0"], b0)
    assert want["steps"] == ref["steps"] and want["buffloc"] == ref["buffloc"] + b0
    assert all(np.array_equal(a, b) for a, b in zip(want["hsel"], ref["hsel"])) and want["edge"] == ref["edge"]
    assert all(want[k] == ref[k] for k in ("flagacq", "iters", "acqcodei", "freqi", "acqfreq", "groups"))


def rule6(sc, chan, r, edge, w0):
    """Rule 6 of DESIGN.md 3.2d on a fetched result `r` and edge of channel `chan` of scenario `sc`, whose span W
    begins at stream sample w0: with the satellite's flip on one of its own period boundaries, inside the deciding
    group and on a hypothesis, buffloc + ((iters // ncoh - 1) * ncoh + edge) * nsamp is where the bit was flipped, to
    the +-1 sample that acqcodei may be off the placed lag; edge 0 says no flip lies inside the deciding group.
    Returns "edge", "none" or None (rule 6 says nothing: not acquired, no hypotheses, a flip off the hypotheses)."""
    prn, _, _, intg, ncoh, estep = chan
    sat = {s[0]: s for s in sc["sats"]}.get(prn)
    if sat is None or not r["flagacq"] or estep == 0:
        return None
    n, lag = cc.nsamp(sc), sat[1]
    assert abs(r["acqcodei"] - lag) <= 1, (chan, r["acqcodei"], lag)
    gstart = r["buffloc"] - r["acqcodei"] + (r["iters"] // ncoh - 1) * ncoh * n     # the deciding group's first sample
    first, end = gstart + lag, gstart + lag + ncoh * n      # the satellite's ncoh periods that the group sums
    flip = w0 + sat[5] if len(sat) > 5 else None
    if flip is None or not first < flip < end:
        assert edge == 0, (chan, "no flip inside the deciding group", edge)
        return "none"
    if (flip - first) % n or ((flip - first) // n) % estep:
        return None
    said = r["buffloc"] + ((r["iters"] // ncoh - 1) * ncoh + edge) * n
    assert edge > 0 and abs(said - flip) <= abs(r["acqcodei"] - lag), (chan, edge, said, flip)
    return "edge"
