"""The scenario of the bit-synchronisation detector's tests (tests/test_bsync_host.py: on the CPU oracle alone, what the
reference's rule and the detector decide; tests/test_gpu_rx_bsync.py: on the device).  Not a conftest.

One ring of int8 IQ at 2.048 Msps, zero IF, 3 s pushed in chunks of 0.25 s with one scheduling step each, four L1 C/A
channels from SEARCH, every satellite's bits tied to its code (synth.make_if, symbol_periods 20) and chosen here:
  A  PRN 12 (checksync()'s shift-register branch), 48 dB-Hz.  The tracker's periods cnt 2001 .. 2020, the first twenty
     the reference's rule looks at, fall into two bits that were sent alike: it synchronises at cnt 2020 on an edge that
     is half a bit off.
  B  PRN 23 (the same branch), 47 dB-Hz, the same geometry with a transition inside those periods.
  C  PRN 3 (the vote branch, prn <= 5), 50 dB-Hz.
  -  PRN 9, absent: never acquired.

Geometry.  A hand-over at sample b starts row 0 (cnt 0) at code period P = round((codephase + rate*b/f_sf) / 1023) of
the absolute code phase; row e holds code period P + e of bit (P + e) // 20, and the true synci is (19 - P) mod 20.
The searches are exact, so the hand-overs are those of the oracle: P0 below, which tests/test_bsync_host.py asserts.
Each code phase carries whole code periods (1023 k chips) that put P0 mod 20 at 9: the bit edge in the middle of the
periods 2001 .. 2020.

Bits.  All bits alternate except where stated: every bit has a transition on both sides, so that the alignment half a
bit away collects next to nothing and the deciding ratio is far from any gate.  A: the two bits that hold the periods
2001 .. 2020 are alike.  Bits are indexed by the absolute code phase, bit s = code periods 20 s .. 20 s + 19."""
import ctypes as C

import numpy as np

import bsync_restate as br
import rx_cases as rc

F_SF, NSAMP = 2.048e6, 2048
F_CF, CRATE, CLEN = 1575.42e6, 1.023e6, 1023
RATE = 20
TAPS = dict(corrn=2, corrd=1, corrp=1)
CHUNK = int(0.25 * F_SF)                        # samples per push: 250 code periods
DURATION = 3.0
NCHUNK = int(DURATION / 0.25)
MAX_PERIODS = 300
RETRY_MS = 1500
INTG = 10
FIRST_TRY = (INTG + 1) * NSAMP
SEED = 2048
NBITS = 160
# (prn, Doppler Hz, code phase chips below one period, whole periods added, C/N0 dB-Hz, carrier phase)
SATS = [(12, -1130.0, 311.3, 9, 48.0, 0.4), (23, 2105.0, 640.7, 9, 47.0, 1.9), (3, 517.0, 12.8, 9, 50.0, 3.3)]
ABSENT = 9
PRNS = [s[0] for s in SATS] + [ABSENT]          # channel order: A, B, C, the absent one
NAMES = "ABC-"
# the code period of row 0 after the first search (step 0, write position CHUNK): measured on the oracle, asserted by
# tests/test_bsync_host.py::test_control_reference_rule_on_the_oracle
P0 = (249, 249, 249)

# the detector's parameters, chosen from the oracle's measurements (tests/test_bsync_host.py asserts the room; DESIGN.md
# 3.2g has the table): tests every NSYM bits from START_CNT on
START_CNT, NSYM, NSYM_MAX, GATE = 200, 25, 100, 3.0
PRM = dict(start_cnt=START_CNT, nsym=NSYM, nsym_max=NSYM_MAX, gate=GATE)
# the same for the SBAS channels of tests/lock_sbas_cases.py (rate 2, random symbols: the ratio is just below 2)
SBAS_PRM = dict(start_cnt=200, nsym=100, nsym_max=400, gate=1.4)


def codephase(i):
    return SATS[i][2] + CLEN * SATS[i][3]


def bits(i):
    """The +-1 bits satellite i sends, by bit number of the absolute code phase."""
    b = np.where(np.arange(NBITS) % 2 == 0, 1.0, -1.0)
    s = (P0[i] + 2001) // RATE                   # the bit that holds cnt 2001
    if i == 0:
        b[s + 1] = b[s]                          # A: sent alike (the bits behind keep alternating from there)
        b[s + 2:] = -b[s + 2:]
    return b


def true_synci(i, p0=None):
    return br.layout_synci(P0[i] if p0 is None else p0, 0, RATE)


def sats():
    return [dict(prn=p, doppler=d, codephase=codephase(i), cn0=cn0, phase=ph, bits=bits(i), symbol_periods=RATE)
            for i, (p, d, _, _, cn0, ph) in enumerate(SATS)]


_SIGNAL = []


def signal(gc, synth):
    """The recording, generated once per process."""
    if not _SIGNAL:
        codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in PRNS}
        _SIGNAL.append(synth.make_if(codes, NCHUNK * CHUNK, f_sf=F_SF, f_if=0.0, dtype=2, sats=sats(), seed=SEED))
    return _SIGNAL[0]


def channels(gc):
    return [gc.Channel(p, dtype=2, f_sf=F_SF, f_if=0.0, **TAPS) for p in PRNS]


def step_wrpos():
    return [CHUNK * (k + 1) for k in range(NCHUNK)]


def code_period(i, buffloc):
    """The code period of the absolute code phase that starts at the hand-over sample `buffloc` of satellite i."""
    rate = CRATE * (1.0 + SATS[i][1] / F_CF)
    x = (codephase(i) + rate * buffloc / F_SF) / CLEN
    assert abs(x - round(x)) < 0.02, x           # the hand-over is on a code epoch to a few hundredths of a period
    return int(round(x))


def sent_bits(i, p0, cnts):
    """The bits satellite i sent in the bit periods that end at the tracker's periods `cnts` (row 0 = code period p0)."""
    b = bits(i)
    return [int(b[(p0 + int(c)) // RATE]) for c in cnts]


def oracle_run(gc, orc, sig, i, prm=None, poke_steps=True, wrpos=None, max_periods=MAX_PERIODS, force=False, chan=None):
    """Channel i on the oracle alone, free-running: orc_sdracquisition at every step until it acquires, then
    orc_sdrthread_step for up to max_periods periods per step.  prm: the detector's parameters (None: the reference's
    rule alone); the restated detector runs over each step's rows, and a decision is poked into the oracle --
    flagsync = 1, synci -- at the next step boundary, as the schedule does.  Returns dict(handover=buffloc or None,
    rows=dict of arrays over all tracked periods (cnt, I, Q, flagsync, navbit), sync=(cnt, synci) of the row in which
    flagsync rose or None, st=the detector's state, events=its tests, poked=step of the poke or None).  force: a failed
    first search hands over all the same, at the sample and the frequency of its best cell: the tracker then runs on
    noise (the absent PRN, which the schedule never tracks).  chan: another scenario's channel instead of channel i,
    dict(prn, ctype, f_sf, nsamp, rate, taps, first_try)."""
    L = orc.lib()
    ring = orc.make_ring(sig, sig.shape[0], 0)
    ch = chan or dict(prn=PRNS[i], ctype=1, f_sf=F_SF, nsamp=NSAMP, rate=RATE, taps=TAPS, first_try=FIRST_TRY)
    mk = lambda: orc.make_chan(ch["prn"], ctype=ch["ctype"], dtype=2, f_sf=ch["f_sf"], f_if=0.0, **ch["taps"])
    o = mk()
    assert (o.rate, o.nsamp) == (ch["rate"], ch["nsamp"])
    b = C.c_uint64(0)
    out = dict(handover=None, sync=None, poked=None, events=[], st=br.zero_state())
    rows = dict(cnt=[], I=[], Q=[], flagsync=[], navbit=[])
    pending = None
    for k, wp in enumerate(step_wrpos() if wrpos is None else wrpos):
        if out["handover"] is None:
            if wp < ch["first_try"]:
                continue
            o = mk()
            loc, _ = rc.oracle_search(orc, o, ring, wp)
            if not o.flagacq:
                if not force:
                    continue
                o.flagacq, o.carrfreq, o.codefreq = 1, o.acq.acqfreq, o.crate
            out["handover"] = loc
            b.value = loc
        if pending is not None and poke_steps:
            if not o.flagsync:
                o.flagsync, o.synci = 1, pending
                out["poked"] = k
            pending = None
        ring.wrpos = wp
        n0, cnt0 = len(rows["I"]), int(o.cnt)
        while len(rows["I"]) - n0 < max_periods and L.orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(b)):
            rows["cnt"].append(int(o.cnt) - 1)
            rows["I"].append(o.II[0])
            rows["Q"].append(o.QQ[0])
            rows["flagsync"].append(o.flagsync)
            rows["navbit"].append(o.bit if (o.flagsync and o.swsync) else 0)
            if o.flagsync and out["sync"] is None:
                out["sync"] = (int(o.cnt) - 1, int(o.synci))
        if prm is not None:
            was = out["st"]["done"]
            br.run(out["st"], prm, ch["rate"], rows["I"][n0:], rows["Q"][n0:], rows["flagsync"][n0:], len(rows["I"]) - n0, cnt0,
                   events=out["events"])
            if out["st"]["done"] == 1 and was == 0:
                pending = out["st"]["synci"]
    out["rows"] = {k: np.array(v) for k, v in rows.items()}
    return out
