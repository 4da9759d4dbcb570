"""gnsscorr_sync_* on constructed rows, no GPU: the library against the literal restatement tests/sync_restate.py, every
field of every epoch row bit for bit after every call (IEEE doubles, the same operations in the same order; the library
is built with -ffp-contract=off), and against what the rows were built to hold: satellites at chosen delays, whose
pseudorange differences are CLIGHT times the delay differences.  Each quirk of the reference that the library keeps
 has a test here that states what a tidier implementation would give instead.
Memory safety: the stand-alone program tests/host/sync_host.c with csrc/sdr_sync.c alone, plain and under address and
undefined-behaviour sanitizers, run as a child process.

The rows.  One stream at 4.092 Msps, 4092 samples per code period, rows every 10 periods (loopms 10).  A satellite at
delay d begins its code period cnt at the real-valued sample x = (d + cnt/1000) * f_sf, kept exact as a Fraction;
the row holds codei = ceil(x) and remcout = codei - x rounded once, so codei - remcout is where the period began, as
in setobsdata() (ref src/sdrtrk.c:167-170).  tow = firstsftow + (double)(cnt - firstsfcnt) * ctime in the library's
own operations (csrc/sdr_host.c), so all satellites share cnt for one tow."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import sync_restate as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SF, NSAMP, CTIME = 4.092e6, 4092, 1e-3
TI = 1 / F_SF
FSFTOW, FSFCNT = 420006.0, 8300                 # the frame's end: its time of week and period counter
WEEK = 2262
DELAYS = (Fraction(0), Fraction(43, 10000), Fraction(117, 10000))      # s: 0, 4.3 and 11.7 ms


def start_sample(delay, cnt):
    return (delay + Fraction(cnt, 1000)) * Fraction(4092000)


def make_rows(delay, cnts, firstsftow=FSFTOW, firstsfcnt=FSFCNT, dop=1000.0, seed=1, snr_at=lambda k: k % 10 == 0, s_of=None):
    """Rows of one satellite for the period counters `cnts` (dicts of sr.ROW_FIELDS)."""
    rng = np.random.default_rng(seed)
    rows, L = [], 0.25 * seed
    for k, cnt in enumerate(cnts):
        x = start_sample(delay, cnt)
        codei = math.ceil(x)
        D = -dop + float(rng.normal(0.0, 0.3))
        L += D * 0.01
        snr = int(bool(snr_at(k)))
        S = (s_of(k) if s_of else 40.0 + 0.001 * k) if snr else 0.0
        rows.append(dict(tow=firstsftow + sr.u2d(cnt - firstsfcnt) * CTIME, remcout=float(codei - x), L=L, D=D, S=S,
                         codei=codei, cntout=cnt, snr=snr))
    return rows


def frame(flagdec=1, week=WEEK, firstsfcnt=FSFCNT, firstsf=None, delay=Fraction(0)):
    firstsf = math.ceil(start_sample(delay, firstsfcnt)) if firstsf is None else firstsf
    return dict(flagdec=flagdec, week=week, firstsf=firstsf, firstsfcnt=firstsfcnt)


def as_array(gc, rows):
    a = np.zeros(len(rows), dtype=np.dtype(gc.ObsRow))
    for n in sr.ROW_FIELDS:
        a[n] = [r[n] for r in rows]
    return a


def setup3(delays=DELAYS):
    return [("chan", i, NSAMP, CTIME, TI) for i in range(len(delays))]


def run_ops(gc, nch, outms, ops):
    """The library and the restatement through the same calls, compared after each; returns all epoch rows (tuples in the
    order of sr.OUT_FIELDS)."""
    lib, rep, out = gc.Sync(nch, outms), sr.SyncRestate(nch, outms), []
    try:
        for op in ops:
            if op[0] == "chan":
                lib.channel(*op[1:])
                rep.channel(*op[1:])
            elif op[0] == "push":
                lib.push(op[1], gc.SyncFrame(**op[2]), as_array(gc, op[3]))
                rep.push(op[1], op[2], op[3])
            elif op[0] == "detach":
                lib.detach(op[1])
                rep.detach(op[1])
            else:
                lib.flush()
                rep.flush()
            got = sr.out_of(lib.fetch())
            assert sr.same_bits(got, rep.out[len(out):]), op[:2]
            out += got
    finally:
        lib.close()
    return out


def kof(tow):
    """The row number (10 ms steps from the frame's end) of an epoch's tow."""
    return round((tow - sr.PTIMING / 1000 - FSFTOW) * 100)


def epochs(out):
    """[(tow, {ch: row dict})] of a list of epoch rows."""
    eps = []
    for r in out:
        d = dict(zip(sr.OUT_FIELDS, r))
        if not eps or eps[-1][0] != d["tow"]:
            eps.append((d["tow"], {}))
        eps[-1][1][d["ch"]] = d
    return eps


def p_bound(nmax):
    """The rounding bound of one P = (CLIGHT*ti) * ((double)(codei - sampref) - remcout), from codei*ti in fp64: the
    integer difference N = codei - sampref is exact (|N| <= nmax < 2^53 samples), remcout was rounded once (|err| <= 2^-53
    since remcout < 1), N - remcout rounds by half an ulp of nmax, and ti = 1/f_sf, CLIGHT*ti and the product round once
    each, 3 * 2^-53 of |P| <= CLIGHT*ti*nmax together (first order)."""
    u = 2.0 ** -53
    return sr.CLIGHT * TI * (math.ulp(float(nmax)) / 2 + u) + 3 * u * sr.CLIGHT * TI * nmax


def check_truth(out, delays, chans=None):
    """Per epoch and pair of satellites: P_i - P_j against CLIGHT * (delay_i - delay_j), compared exactly (Fractions of the
    doubles) within the derived bound.  Returns the worst |error| / bound."""
    worst = 0.0
    for tow, sat in epochs(out):
        chs = sorted(sat) if chans is None else [c for c in sorted(sat) if c in chans]
        bound = 2 * p_bound(100 * NSAMP)        # |codei - sampref| stays below 68.802 + 11.7 + 10 ms of samples
        for i in chs:
            for j in chs:
                err = Fraction(sat[i]["P"]) - Fraction(sat[j]["P"]) - Fraction(sr.CLIGHT) * (delays[i] - delays[j])
                assert abs(err) <= Fraction(bound), (tow, i, j, float(err), bound)
                worst = max(worst, float(abs(err)) / bound)
    return worst


# ---- layout and refusals ---------------------------------------------------------------------------------------------
def test_layout_and_constants(gc):
    assert C.sizeof(gc.SyncFrame) == 24 and C.sizeof(gc.EpochObs) == 56 and gc.EpochObs.sampref.offset == 48
    assert (gc.OBSHIST, gc.PTIMING, gc.SYNCQCAP) == (sr.NH, sr.PTIMING, sr.QCAP) == (80, 68.802, 4096)
    hdr = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    for text in ("GNSSCORR_OBSHIST   80", "GNSSCORR_PTIMING   68.802", "GNSSCORR_SYNCQCAP  4096"):
        assert text in hdr


def test_every_refusal_touches_nothing(gc):
    """Each refusal is GNSSCORR_EINVAL with a message; after all of them the state gives the epochs of a fresh one."""
    L = gc.lib()
    gc.Sync(1, 10).close()                      # (binds the argument types)
    h = C.c_void_p()
    assert L.gnsscorr_sync_create(None, 3, 10) == gc.EINVAL
    for nch, outms in [(0, 10), (-1, 10), (3, 0), (3, -10)]:
        assert L.gnsscorr_sync_create(C.byref(h), nch, outms) == gc.EINVAL and not h
    rows = make_rows(DELAYS[0], range(FSFCNT, FSFCNT + 400, 10))
    arr, fr = as_array(gc, rows), gc.SyncFrame(**frame())
    s = gc.Sync(3, 10)

    def refused(f, *a):
        with pytest.raises(gc.GnsscorrError) as e:
            f(*a)
        assert e.value.code == gc.EINVAL and str(e.value)

    assert L.gnsscorr_sync_channel(None, 0, NSAMP, CTIME, TI) == gc.EINVAL
    assert L.gnsscorr_sync_push(None, 0, C.byref(fr), arr.ctypes.data, 1) == gc.EINVAL
    assert L.gnsscorr_sync_detach(None, 0) == gc.EINVAL and L.gnsscorr_sync_flush(None) == gc.EINVAL
    assert L.gnsscorr_sync_fetch(None, arr.ctypes.data, 1) == gc.EINVAL
    refused(s.push, 0, fr, arr[:1])             # before gnsscorr_sync_channel
    for ch in (-1, 3):
        refused(s.channel, ch, NSAMP, CTIME, TI)
        refused(s.push, ch, fr, arr[:1])
        refused(s.detach, ch)
    for bad in [(0, CTIME, TI), (NSAMP, 0.0, TI), (NSAMP, CTIME, 0.0), (NSAMP, math.nan, TI), (NSAMP, CTIME, math.inf)]:
        refused(s.channel, 0, *bad)
    s.channel(0, NSAMP, CTIME, TI)
    refused(s.channel, 1, NSAMP, CTIME, 1 / 4.0e6)      # another ti
    assert L.gnsscorr_sync_push(s.h, 0, None, arr.ctypes.data, 1) == gc.EINVAL
    assert L.gnsscorr_sync_push(s.h, 0, C.byref(fr), None, 1) == gc.EINVAL
    assert L.gnsscorr_sync_push(s.h, 0, C.byref(fr), arr.ctypes.data, -1) == gc.EINVAL
    assert L.gnsscorr_sync_fetch(s.h, None, 1) == gc.EINVAL and L.gnsscorr_sync_fetch(s.h, arr.ctypes.data, -1) == gc.EINVAL
    s.push(0, fr, arr[:20])
    refused(s.push, 0, fr, arr[19:21])          # codei equal to the channel's last
    refused(s.push, 0, fr, arr[[20, 22, 21]])   # not ascending within the push: none of it is taken
    s.push(0, fr, arr[20:])
    got = sr.out_of(s.fetch())
    s.close()
    want = run_ops(gc, 3, 10, [("chan", 0, NSAMP, CTIME, TI), ("push", 0, frame(), rows)])
    assert len(want) > 20 and sr.same_bits(got, want)


def test_queue_cap_names_the_channel_that_holds_the_others_back(gc):
    rows = make_rows(DELAYS[0], range(FSFCNT, FSFCNT + 10 * (sr.QCAP + 1), 10))
    arr, fr = as_array(gc, rows), gc.SyncFrame(**frame())
    s = gc.Sync(3, 10)
    for ch in (0, 2):
        s.channel(ch, NSAMP, CTIME, TI)
    s.push(0, fr, arr[:sr.QCAP])                # channel 2 has nothing yet: all of it waits
    assert len(s.fetch()) == 0
    with pytest.raises(gc.GnsscorrError) as e:
        s.push(0, fr, arr[sr.QCAP:])
    assert e.value.code == gc.ESTATE and "channel 2 holds the others back" in str(e.value)
    s.detach(2)                                 # nothing was touched: the 4096 rows are consumed now, then the refused one
    n = len(s.fetch())
    s.push(0, fr, arr[sr.QCAP:])
    got = n + len(s.fetch())
    s.close()
    want = run_ops(gc, 1, 10, [("chan", 0, NSAMP, CTIME, TI), ("push", 0, frame(), rows[:2000]), ("push", 0, frame(), rows[2000:])])
    assert got == len(want) > 4000


# ---- full histories, the truth, the grid -----------------------------------------------------------------------------
def three_full(nrow=140, fsftow=FSFTOW):
    """Three satellites: 90 rows before the frame is known (flagdec 0), then rows with it: every epoch sees full
    histories."""
    ops = setup3()
    first = FSFCNT - 900
    for i, d in enumerate(DELAYS):
        rows = make_rows(d, range(first, first + 10 * nrow, 10), firstsftow=fsftow, dop=1000.0 * (i - 1), seed=i + 1)
        ops += [("push", i, frame(flagdec=0), rows[:90]), ("push", i, frame(), rows[90:])]
    return ops + [("flush",)]


def test_three_channels_full_histories_and_truth(gc):
    out = run_ops(gc, 3, 10, three_full())
    eps = epochs(out)
    # (the nearest satellite is eligible first: the epoch of its first row with the frame holds it alone)
    assert len(eps) >= 40 and sorted(eps[0][1]) == [0] and all(sorted(sat) == [0, 1, 2] for _, sat in eps[1:])
    worst = check_truth(out, DELAYS)
    print("worst |P_i - P_j - truth| / bound = %.3f (bound %.3g m)" % (worst, 2 * p_bound(100 * NSAMP)))
    for tow, sat in eps[1:]:
        k = kof(tow)
        assert tow == FSFTOW + sr.u2d(10 * k) * CTIME + sr.PTIMING / 1000
        for i in range(3):
            assert sat[i]["week"] == WEEK and abs(sat[i]["D"] + 1000.0 * (i - 1)) < 2.0 and 40.0 <= sat[i]["S"] < 41.0
            assert sat[i]["sampref"] == sat[0]["sampref"]
        # the nearest satellite (delay 0) is the reference: sampref lies 68.802 ms before its row of this tow
        assert sat[0]["sampref"] == math.ceil(start_sample(DELAYS[0], FSFCNT)) + int(NSAMP * (-68.802 + 10.0 * k))


@pytest.mark.parametrize("fsftow", [258.0, 4098.0])
@pytest.mark.parametrize("outms", [10, 100])
def test_truncation_drops_epochs_quirk_b(gc, outms, fsftow):
    """(int)(reftow*1000) % outms: where the product falls just below an integer the epoch is dropped.  The naive count is
    one epoch per row of the most distant satellite whose rounded millisecond lies on the grid.  Early in the week, where
    a tow has bits to spare behind the millisecond, 48 of these 200 products fall low (4 of the 20 on the 100 ms grid); at
    420006 s none of them does."""
    out = run_ops(gc, 3, outms, three_full(nrow=290, fsftow=fsftow))
    got = [t for t, _ in epochs(out)]
    tows = [fsftow + sr.u2d(10 * k) * CTIME for k in range(200)]                # the rows with the frame known
    naive = [t for t in tows if round(t * 1000) % outms == 0]
    kept = [t for t in naive if int(t * 1000) % outms == 0]
    assert got == [t + sr.PTIMING / 1000 for t in kept]
    assert len(naive) == 200 * 10 // outms and len(naive) - len(kept) == (48 if outms == 10 else 4)
    print("outms %d: %d epochs of %d" % (outms, len(kept), len(naive)))


# ---- quirk (c): short histories ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhist", [5, 79, 81])
def test_short_histories_quirk_c(gc, nhist):
    """The epoch made when the histories hold nhist rows: sampbase reads codei[79], 0 while fewer than 80 rows are there,
    and wraps.  With 5 rows the interpolation point (68.802 ms back) lies before the oldest row, so the three points are the
    two oldest rows and an unfilled element (L = D = 0 at abscissa 10*nsamp): the most distant satellite's Doppler comes
    out 6 to 11 Hz off its -1000 +- 1, where a tidier implementation would use the rows it has.  The very first epoch (one
    row, one satellite) takes its three points among equal abscissae and divides by zero: NaN.  In epoch 78 the nearest
    satellite, the reference, has its 80th row and the others have 79: sampbase is a real sample count now, their
    codei[79] = 0 wraps to an abscissa near 2^64 at the wrong end of the descending list, and their Doppler is 10 to 25 Hz
    off; one epoch later all is in order.  P does not depend on sampbase and is the truth throughout."""
    ops = setup3()
    for i, d in enumerate(DELAYS):
        ops.append(("push", i, frame(), make_rows(d, range(FSFCNT, FSFCNT + 10 * (nhist + 2), 10), seed=i + 1)))
    out = run_ops(gc, 3, 10, ops)
    check_truth(out, DELAYS)
    eps = epochs(out)
    assert kof(eps[-1][0]) == nhist - 1 and sorted(eps[0][1]) == [0] and math.isnan(eps[0][1][0]["L"]) and math.isnan(eps[0][1][0]["D"])
    for tow, sat in eps[1:]:
        off = [abs(sat[i]["D"] + 1000.0) for i in range(3)]
        if kof(tow) < 5:
            assert 5.0 < off[2] < 12.0
        elif kof(tow) < 8:
            pass                                # (the unfilled element leaves the three points: 68.802 ms are 7 rows)
        elif kof(tow) == 78:
            assert off[0] < 2.0 and 5.0 < off[1] < 30.0 and 5.0 < off[2] < 30.0
        else:
            assert max(off) < 2.0, kof(tow)


# ---- the wrap definition -------------------------------------------------------------------------------------------------
def test_first_68_periods_after_the_frame_end(gc):
    """cntout - firstsfcnt < 69: nsamp*(-68.802 + diffcnt) is negative; converted to int64 and added modulo 2^64, sampref
    lies before firstsf.  firstsf = 100 samples makes the sum itself pass below zero and wrap."""
    ops = setup3()
    for i, d in enumerate(DELAYS):
        ops.append(("push", i, frame(), make_rows(d, range(FSFCNT, FSFCNT + 120, 10), seed=i + 1)))
    out = run_ops(gc, 3, 10, ops + [("flush",)])
    fsf = math.ceil(start_sample(DELAYS[0], FSFCNT))
    eps = epochs(out)
    early = [sat for tow, sat in eps if tow < FSFTOW + 0.068 + sr.PTIMING / 1000]
    assert len(early) >= 6 and all(sat[0]["sampref"] < fsf for sat in early)
    assert [sat[0]["sampref"] for _, sat in eps][:3] == [fsf + int(NSAMP * (-68.802 + 10.0 * k)) for k in range(3)]
    check_truth(out, DELAYS)
    rows = make_rows(Fraction(0), range(0, 50, 10), firstsftow=6.0, firstsfcnt=0)
    out = run_ops(gc, 1, 10, [("chan", 0, NSAMP, CTIME, TI), ("push", 0, frame(firstsfcnt=0, firstsf=100), rows)])
    assert out[0][7] == (100 + int(NSAMP * -68.802)) % 2 ** 64 > 2 ** 63


# ---- quirk (d): S ----------------------------------------------------------------------------------------------------------
def test_s_is_the_newest_quirk_d(gc):
    """Satellite 0 (nearest) is one row ahead when the most distant one completes an epoch, so its ind is 1; its rows carry
    an S every third row, out of step with the epochs.  The epoch holds the S set last -- at times by the row at [0],
    newer than the row at ind the pseudorange is taken from -- not the S of the row at ind (0.0 for most rows)."""
    s_of = lambda k: 30.0 + k
    ops = setup3((DELAYS[0], DELAYS[2]))
    cnts = range(FSFCNT, FSFCNT + 300, 10)
    ops.append(("push", 0, frame(), make_rows(DELAYS[0], cnts, seed=1, snr_at=lambda k: k % 3 == 1, s_of=s_of)))
    ops.append(("push", 1, frame(), make_rows(DELAYS[2], cnts, seed=2)))
    eps = epochs(run_ops(gc, 2, 10, ops))
    assert len(eps) >= 25
    newer = 0
    for tow, sat in eps[1:]:
        n = kof(tow)                            # the epoch of row n: satellite 0 has consumed row n + 1
        newest = max(k for k in range(n + 2) if k % 3 == 1)
        assert sat[0]["S"] == s_of(newest)
        newer += newest == n + 1
    assert newer >= 8


# ---- quirk (a): ind by position, kept -----------------------------------------------------------------------------------
def test_stale_ind_by_position_quirk_a(gc):
    """ind[] belongs to the position in the eligible list and keeps its value when no history element matches reftow.
    Satellites 0 and 1 are distant (11.7 and 11.0 ms), satellite 2 near (0 ms): when 0 completes an epoch, 2 is a row
    ahead, so ind = [0, 0, 1].  Then channel 1 loses eligibility (a push with flagdec 0) and channel 2 is detached and
    attaches again with the row one after the next epoch's.  In that epoch the list is [0, 2]; channel 2's history holds
    no row of reftow, so its ind is what position 1 had: 0, channel 1's.  Its pseudorange is taken from its only row, 10 ms
    late.  An ind kept per channel would give 1 (an empty element), and a tidy poll would leave the satellite out."""
    delays = (DELAYS[2], Fraction(110, 10000), Fraction(0))
    ops = setup3(delays)
    a, b, c = FSFCNT, FSFCNT + 200, FSFCNT + 400
    for i, d in enumerate(delays):
        ops.append(("push", i, frame(), make_rows(d, range(a, b, 10), seed=i + 1)))
    steady = epochs(run_ops(gc, 3, 10, ops))
    assert len(steady) >= 18 and sorted(steady[-1][1]) == [0, 1, 2]
    ops.append(("detach", 2))
    ops.append(("push", 1, frame(flagdec=0), make_rows(delays[1], range(b, c, 10), seed=2)))
    ops.append(("push", 2, frame(), make_rows(delays[2], range(b + 10, c, 10), seed=3)))
    ops.append(("push", 0, frame(), make_rows(delays[0], range(b, c, 10), seed=1)))
    out = run_ops(gc, 3, 10, ops + [("flush",)])
    eps = epochs(out)
    at = [n for n, (tow, _) in enumerate(eps) if kof(tow) == (b - FSFCNT) // 10]
    assert len(at) == 1 and all(sorted(sat) == [0, 1] for _, sat in eps[len(steady):at[0]])    # (while channel 2 was away)
    eps = eps[at[0]:]
    first = eps[0][1]
    assert sorted(first) == [0, 2]
    late = first[2]["P"] - first[0]["P"] - float(sr.CLIGHT * (delays[2] - delays[0]))
    assert abs(late - sr.CLIGHT * 0.010) < 1e-3                      # channel 2's row of tow + 10 ms
    # from the next epoch on channel 2 has the row of reftow and the truth is back
    assert all(sorted(sat) == [0, 2] for _, sat in eps[1:]) and len(eps) >= 15
    check_truth([r for r in out if r[2] > eps[0][0]], delays, chans=(0, 2))


def test_a_channel_becomes_eligible_mid_stream(gc):
    """Channel 1 decodes its frame 100 periods after the others: from its first eligible row on the epochs hold three
    satellites, in channel order, and the positions of channels behind it shift by one."""
    ops = setup3()
    cnts = range(FSFCNT, FSFCNT + 300, 10)
    for i, d in enumerate(DELAYS):
        rows = make_rows(d, cnts, seed=i + 1)
        if i == 1:
            ops += [("push", 1, frame(flagdec=0), rows[:10]), ("push", 1, frame(week=0), rows[10:12]), ("push", 1, frame(), rows[12:])]
        else:
            ops.append(("push", i, frame(), rows))
    out = run_ops(gc, 3, 10, ops + [("flush",)])
    eps = epochs(out)
    # the nearest satellite is alone for its first two rows; the most distant one's first row (11.7 ms behind) then takes
    # reftow back: the epochs of rows 0 and 1 are made a second time with two satellites, as the reference would
    want = [(0, [0]), (1, [0])] + [(k, [0, 2]) for k in range(12)] + [(k, [0, 1, 2]) for k in range(12, 30)]
    assert [(kof(tow), sorted(sat)) for tow, sat in eps] == want
    check_truth(out, DELAYS)


# ---- cuts and interleavings --------------------------------------------------------------------------------------------
def cut_ops(seed, per_chan):
    """The rows of every channel cut at random places, the pieces of the channels interleaved at random."""
    rng = np.random.default_rng(seed)
    pieces = []
    for i, (fr_rows) in enumerate(per_chan):
        mine = []
        for fr, rows in fr_rows:                # (a push never spans two frame states)
            cuts = sorted(set(rng.integers(1, len(rows), size=rng.integers(0, 8)).tolist())) if len(rows) > 1 else []
            for a, b in zip([0] + cuts, cuts + [len(rows)]):
                mine.append(("push", i, fr, rows[a:b]))
        pieces.append(mine)
    ops = []
    while any(pieces):
        i = int(rng.choice([k for k, p in enumerate(pieces) if p]))
        ops.append(pieces[i].pop(0))
    return ops


def whole_and_cut_cases():
    per_chan = []
    for i, d in enumerate(DELAYS):
        rows = make_rows(d, range(FSFCNT - 300, FSFCNT + 900, 10), dop=700.0 * (i - 1), seed=i + 1)
        per_chan.append([(frame(flagdec=0), rows[:30]), (frame(), rows[30:])])
    return per_chan


def test_output_does_not_depend_on_cuts_and_interleavings(gc):
    per_chan = whole_and_cut_cases()
    whole = setup3() + [("push", i, fr, rows) for i, fr_rows in enumerate(per_chan) for fr, rows in fr_rows] + [("flush",)]
    want = run_ops(gc, 3, 10, whole)
    assert len(epochs(want)) >= 60
    for seed in range(20):
        got = run_ops(gc, 3, 10, setup3() + cut_ops(seed, per_chan) + [("flush",)])
        assert sr.same_bits(got, want), seed
    reverse = setup3() + [("push", i, fr, rows) for i, fr_rows in reversed(list(enumerate(per_chan))) for fr, rows in fr_rows]
    assert sr.same_bits(run_ops(gc, 3, 10, reverse + [("flush",)]), want)


# ---- the stand-alone program -------------------------------------------------------------------------------------------
def script_of(nch, outms, ops):
    lines = ["create %d %d" % (nch, outms)]
    for op in ops:
        if op[0] == "chan":
            lines.append("chan %d %d %s %s" % (op[1], op[2], float(op[3]).hex(), float(op[4]).hex()))
        elif op[0] == "push":
            fr = op[2]
            lines.append("push %d %d %d %d %d %d" % (op[1], fr["flagdec"], fr["week"], fr["firstsf"], fr["firstsfcnt"], len(op[3])))
            for r in op[3]:
                lines.append(" ".join([float(r[n]).hex() for n in ("tow", "remcout", "L", "D", "S")] +
                                      ["%d %d %d" % (r["codei"], r["cntout"], r["snr"])]))
        elif op[0] == "detach":
            lines.append("detach %d" % op[1])
        else:
            lines.append("flush")
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("synchost") / ("sync_host_" + request.param))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                      "-static-libasan", "-static-libubsan"]      # (no runtime to load first)
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                          [os.path.join(ROOT, "tests", "host", "sync_host.c"),
                           os.path.join(ROOT, "erlangnetwork-gnsslib-sdr_amd", "csrc", "sdr_sync.c"), "-o", exe, "-lm"])
    return exe


def run_exe(exe, tmp_path, nch, outms, ops):
    path = tmp_path / "script.txt"
    path.write_text(script_of(nch, outms, ops))
    res = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    rcs, out = [], []
    for line in res.stdout.splitlines():
        t = line.split()
        if t[0] == "rc":
            rcs.append(int(t[1]))
        else:
            out.append((int(t[0]), int(t[1])) + tuple(float.fromhex(v) for v in t[2:7]) + (int(t[7]),))
    return rcs, out


def test_standalone_program_on_the_cut_and_interleave_case(gc, host_exe, tmp_path):
    """csrc/sdr_sync.c linked alone with its driver (once plain, once under the sanitizers): a cut and interleaved input
    with a detach, short histories and a refused push in it, against the restatement."""
    per_chan = whole_and_cut_cases()
    ops = setup3() + cut_ops(5, per_chan)
    more = [make_rows(d, range(FSFCNT + 900, FSFCNT + 1200, 10), seed=i + 7) for i, d in enumerate(DELAYS)]
    ops += [("detach", 1), ("push", 0, frame(), more[0]), ("push", 2, frame(), more[2][:9]), ("push", 2, frame(), more[2][8:]),
            ("push", 1, frame(), more[1][20:]), ("push", 2, frame(), more[2][9:]), ("flush",)]
    rcs, out = run_exe(host_exe, tmp_path, 3, 10, ops)
    bad = len(ops) - 4 + 1                      # (+ 1: the create line)
    assert rcs == [0] * bad + [gc.EINVAL] + [0] * 3
    rep = sr.SyncRestate(3, 10)
    for op in ops:
        try:
            getattr(rep, "channel" if op[0] == "chan" else op[0])(*op[1:])
        except ValueError:
            assert op is ops[-4]
    assert len(epochs(out)) >= 100 and sr.same_bits(out, rep.out)
    assert sr.same_bits(out, run_ops(gc, 3, 10, ops[:-4] + ops[-3:]))
