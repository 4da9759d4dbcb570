"""Three L1 C/A satellites in one recording, from IF samples to observation epochs (tests/test_sync_if_host.py holds the
CPU oracle to it, tests/test_gpu_sync_if.py the device; not a conftest): int8 IQ at 4.092 Msps, zero IF, 50 dB-Hz each.
Every satellite carries the same bits, tied to its code (synth.make_if with symbol_periods = 20): LEAD random bits, one
subframe of tests/lnav_frames.py, then random bits.  The satellites differ in delay -- 0, 4.3 and 11.7 ms, as code
phases at t = 0 -- in Doppler and in carrier phase.

Geometry.  A satellite's absolute code phase is phi(t) = codephase + rate*t chips, rate = 1.023e6 (1 + doppler/f_cf);
code period p spans phi in [1023 p, 1023 (p+1)) and bit s the code periods 20 s .. 20 s + 19.  The tracker of a channel
starts at the first code epoch of the recording, code period P0 = ceil(codephase / 1023), on the sample nearest to it,
bit-synchronised with the true carrier: log row e holds code period P0 + e at sdrthread's cnt = cnt0 + e, and synci is
the cnt % 20 of a bit's last period.  The subframe's last bit ends with code period END = 20 (LEAD + 300) - 1: the frame
is found in row END - P0, firstsfcnt = cnt0 + END - P0, firstsftow = 6 TOW_COUNT, and the rows of observables from there
on (every 10 periods) carry tow = firstsftow + 0.01 k.

Truth.  The code epoch that carries tow = firstsftow + 0.01 k is the beginning of code period END + 10 k, phi = 1023 (END
+ 10 k), received from satellite i at t_i = (phi - codephase_i) / rate_i: the pseudoranges of one epoch differ by
CLIGHT (t_i - t_j)."""
import ctypes as C

import numpy as np

F_SF, NSAMP, CTIME = 4.092e6, 4092, 1e-3
F_CF, CRATE, CLEN = 1575.42e6, 1.023e6, 1023
TAPS = dict(corrn=2, corrd=1, corrp=1)
CN0 = 50.0
PRNS = (7, 12, 23)
DELAYS = (0.0, 4.3e-3, 11.7e-3)
DOPPLERS = (1234.0, -2210.0, 3105.0)
PHASES = (0.7, 2.9, 5.1)
CNT0 = (0, 137, 4001)                           # sdrthread's cnt at each channel's row 0
C0 = 12 * CLEN + 200.25                         # chips: the code phase at t = 0 of the satellite without delay
CODEPHASES = tuple(C0 - CRATE * d for d in DELAYS)
LEAD, TAIL = 8, 14
TOW_COUNT, SFID, WEEK = 70001, 2, 2262
END = 20 * (LEAD + 300) - 1                     # the code period that ends the subframe
NROWS_AFTER = 20                                # rows of observables behind the frame's end that every channel reaches
NPER = END + 10 * NROWS_AFTER + 5               # log rows per channel (the channel that starts last begins at P0 = 1)
OUTMS = 10
PIECES = (700, 1300, NPER - 2000)               # the pieces a channel's log is replayed in, and the runs of the cut GPU test
BIT_SEED, SIGNAL_SEED = 99, 7
FIRSTSFTOW = 6.0 * TOW_COUNT


def rate(i):
    return CRATE * (1.0 + DOPPLERS[i] / F_CF)


def p0(i):
    return int(np.ceil(CODEPHASES[i] / CLEN))


def b0(i):
    """The sample nearest to the first code epoch of the recording."""
    return int(round((CLEN * p0(i) - CODEPHASES[i]) / rate(i) * F_SF))


def synci(i):
    return (CNT0[i] + 19 - p0(i)) % 20


def found_row(i):
    return END - p0(i)


def receive_time(i, k):
    """Seconds into the recording at which satellite i's code epoch of tow = firstsftow + 0.01 k arrives."""
    return (CLEN * (END + 10 * k) - CODEPHASES[i]) / rate(i)


def bits():
    from lnav_frames import l1ca_subframe
    rng = np.random.default_rng(BIT_SEED)
    lead = [int(x) for x in rng.choice([-1, 1], size=LEAD)]
    sf, _ = l1ca_subframe(rng, [lead[-2], lead[-1]], TOW_COUNT, SFID, 1)
    return np.array(lead + sf + [int(x) for x in rng.choice([-1, 1], size=TAIL)], np.float64)


def sats():
    b = bits()
    return [dict(prn=PRNS[i], doppler=DOPPLERS[i], codephase=CODEPHASES[i], cn0=CN0, phase=PHASES[i], bits=b, symbol_periods=20)
            for i in range(3)]


_SIGNAL = []


def signal(gc, synth):
    """The recording, generated once per process (NPER + 4 periods: the ring wants a multiple of 8 samples)."""
    if not _SIGNAL:
        codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in PRNS}
        _SIGNAL.append(synth.make_if(codes, NSAMP * (NPER + 4), f_sf=F_SF, f_if=0.0, dtype=2, sats=sats(), seed=SIGNAL_SEED))
    return _SIGNAL[0]


def channels(gc):
    return [gc.Channel(p, dtype=2, f_sf=F_SF, f_if=0.0, **TAPS) for p in PRNS]


_ORACLE = []


def oracle_run(gc, orc, synth):
    """The oracle's closed loop over the recording, free-running from the bit-synchronised state, once per process: per
    channel (log: NPER rows of TrkLog, I: the prompt sum of every row)."""
    if not _ORACLE:
        sig = signal(gc, synth)
        ring = orc.make_ring(sig, sig.shape[0], sig.shape[0])
        L = orc.lib()
        for i, prn in enumerate(PRNS):
            o = orc.make_chan(prn, dtype=2, f_sf=F_SF, f_if=0.0, **TAPS)
            assert (o.rate, o.loopms, o.nsamp) == (20, 10, NSAMP)
            o.acq.acqfreq = DOPPLERS[i]
            o.carrfreq, o.codefreq, o.remcode, o.remcarr = DOPPLERS[i], o.crate, 0.0, 0.0
            o.flagsync, o.synci, o.cnt = 1, synci(i), CNT0[i]
            b = C.c_uint64(b0(i))
            log, I = np.zeros(NPER, dtype=np.dtype(gc.TrkLog)), np.zeros(NPER)
            for e in range(NPER):
                log["buffloc"][e] = b.value
                assert L.orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(b)) == 1
                for n in ("carrfreq", "codefreq", "carrErr", "codeErr", "carrNco", "codeNco", "freqErr", "remcode", "remcarr",
                          "currnsamp", "flagloopfilter", "flagsync"):
                    log[n][e] = getattr(o, n)
                log["navbit"][e] = o.bit if (o.flagsync and o.swsync) else 0
                I[e] = o.II[0]
            _ORACLE.append((log, I))
    return _ORACLE


def replays(gc, i, pieces, I):
    """gnsscorr_frame_replay and gnsscorr_obs_replay over the pieces of channel i's log, as a caller's loop does
    (INTEGRATION.md section 4): the frame state after a piece goes into the observables' state before that piece's rows.
    Returns (frame state, [(SyncFrame, rows of observables)] per piece).  The rows of observables depend on the pieces --
    the row in which the observables' state learns of the frame takes the half cycle of an inverted frame, and sums round
    differently from there on -- so every test here replays in PIECES, however it pushes."""
    fr, st = gc.FrameState(), gc.ObsState()
    st.f_sf, st.f_if, st.foffset, st.ctime, st.loopms = F_SF, 0.0, 0.0, CTIME, 10
    out, a = [], 0
    for rows in pieces:
        gc.frame_replay(fr, rows, cnt0=CNT0[i] + a)
        if fr.flagdec:
            st.flagsyncf, st.polarity, st.firstsftow, st.firstsfcnt = fr.flagsyncf, fr.polarity, fr.firstsftow, fr.firstsfcnt
        obs = gc.obs_replay(st, rows, I[a:a + len(rows)], cnt0=CNT0[i] + a)
        out.append((gc.SyncFrame(int(fr.flagdec), WEEK if fr.flagdec else 0, int(fr.firstsf), int(fr.firstsfcnt)), obs))
        a += len(rows)
    return fr, out


def cut(log):
    edges = np.cumsum((0,) + PIECES)
    assert edges[-1] == len(log)
    return [log[a:b] for a, b in zip(edges[:-1], edges[1:])]


def one_push(i, per_piece):
    """All rows of a channel as one push with the frame the last piece found: the rows before the frame's end are not
    eligible whatever flagdec says (cntout < firstsfcnt)."""
    return (i, per_piece[-1][0], np.concatenate([rows for _, rows in per_piece]))


def restated(pushes):
    """The restatement tests/sync_restate.py through the pushes [(ch, SyncFrame, rows)] and a flush: its epoch rows."""
    import sync_restate as sr
    rep = sr.SyncRestate(3, OUTMS)
    for i in range(3):
        rep.channel(i, NSAMP, CTIME, 1 / F_SF)
    for ch, fr, rows in pushes:
        rep.push(ch, dict(flagdec=fr.flagdec, week=fr.week, firstsf=fr.firstsf, firstsfcnt=fr.firstsfcnt), sr.rows_of(rows))
    rep.flush()
    return rep.out


def library(gc, pushes):
    """The library through the same pushes and one flush: its epoch rows as tuples."""
    import sync_restate as sr
    s = gc.Sync(3, OUTMS)
    try:
        for i, ch in enumerate(channels(gc)):
            s.channel(i, ch.nsamp, ch.ctime, ch.ti)
        for ch, fr, rows in pushes:
            s.push(ch, fr, rows)
        s.flush()
        return sr.out_of(s.fetch())
    finally:
        s.close()


def by_epoch(out):
    """[(tow, {ch: dict of the row})]."""
    import sync_restate as sr
    eps = []
    for r in out:
        d = dict(zip(sr.OUT_FIELDS, r))
        if not eps or eps[-1][0] != d["tow"]:
            eps.append((d["tow"], {}))
        eps[-1][1][d["ch"]] = d
    return eps


def full_epochs(out):
    """The epochs that hold all three satellites, as (k, {ch: row}): tow = FIRSTSFTOW + 0.01 k + 0.068802."""
    import sync_restate as sr
    eps = []
    for tow, sat in by_epoch(out):
        if sorted(sat) == [0, 1, 2]:
            k = round((tow - sr.PTIMING / 1000 - FIRSTSFTOW) * 100)
            assert tow == FIRSTSFTOW + float(10 * k) * CTIME + sr.PTIMING / 1000
            eps.append((k, sat))
    return eps


def worst_range_error(eps):
    """The largest |P_i - P_j - CLIGHT (t_i - t_j)| over the epochs and pairs, metres."""
    import sync_restate as sr
    worst = 0.0
    for k, sat in eps:
        for i in range(3):
            for j in range(i):
                truth = sr.CLIGHT * (receive_time(i, k) - receive_time(j, k))
                worst = max(worst, abs(sat[i]["P"] - sat[j]["P"] - truth))
    return worst

