"""A GLONASS G1 signal that carries strings (synth.make_if with symbol_periods = 10) and what the receiver must find in
it (tests/test_g1_if_host.py holds the CPU oracle to it, tests/test_gpu_g1_if.py the device; not a conftest): frequency
number +1 (562.5 kHz above the front end's centre) on int8 IQ at 2.048 Msps, zero IF, 14 000 code periods: the seven
strings 6, 7, 3, 4, 5, 1, 2 -- a start in mid-frame, the usual case in the field -- tracked from the acquisition
hand-over state with cnt preset just below 2000.

Geometry.  The generator's symbol s lasts while the absolute code phase codephase + rate*t lies in [5110 s, 5110 (s+1)):
code periods 10 s .. 10 s + 9.  The tracker starts at the first code epoch of the recording, code period P0 = 1, which
CODEPHASE puts on a whole sample, so log row e holds code period P0 + e of symbol (P0 + e) // 10, at sdrthread's cnt =
cnt0 + e.  A frequency number <= 5 takes checksync's vote branch (ref src/sdrnav.c:203,218-229): from cnt > 2000 on
every sign change of the prompt sum votes for its cnt % 10, all of them for the first period of a symbol, and the 51st
raises flagsync with synci one before it; checkbit then decides a symbol in every row whose cnt % 10 == synci, the last
period of a sent symbol.  Under the meander every second symbol edge is a sign change for sure and the others one time
in two, so the symbol edge is there long before the first string's time mark.

The frame: string j (0-based) is symbols 200 j .. 200 j + 199, its time mark the last 30; the mark is found in the row
that decides symbol 200 j + 199, row 2000 j + 1999 - P0.  Strings 6 and 7 say no time, so the flags drop after each;
strings 3, 4, 5, 1 bring ephcnt to 4 (and string 1 sets s1cnt = 1), string 2 to 5: the time is merged there with
s1cnt = 2, in the very row its mark was found in, and flagdec rises with firstsftow the GPS time at which string 2
ends."""
import numpy as np

import g1_restate as gr
import g1_strings as gs

F_SF, NSAMP = 2.048e6, 2048
FREQNO, CTYPE_G1 = 1, 20
FOFFSET = 0.5625e6 * FREQNO
DOPPLER, CN0 = -830.0, 47.0                     # (the C/N0 of tests/sbas_if_cases.py)
K0 = 1640                                       # the first code epoch of the recording: a whole sample
CODEPHASE = 511 - K0 * 511 / 2048               # = 101.80078125 chips, exact
TAPS = dict(corrn=2, corrd=1, corrp=1)
RATE = 10
P0, B0 = 1, K0
ACQFREQ = FOFFSET + 200.0 * round(DOPPLER / 200.0)
NOCODEDOPPLER = 1.602e15                        # f_cf given to synth.make_if: the folded FDMA offset is no code Doppler
NUMBERS = [6, 7, 3, 4, 5, 1, 2]
NSYM = 200 * len(NUMBERS)
NPER = RATE * NSYM - P0                         # rows 0 .. NPER-1: the last one closes the last sent symbol
SIGNAL_SEED, STRING_SEED = 201, 77
CNT0 = 1990
# what the strings say: 2023-05-17 14:25:30 Moscow time at the beginning of string 1, satellite slot 9
DATE, TK = (2023, 5, 17), (14, 25, 1)
NT, N4 = gs.glonass_day(*DATE)
SLOT, IODE = 9, 33
WEEK, TOW1 = gs.gps_week_tow(*DATE, TK[0], TK[1], 30 * TK[2])
FIRSTSFTOW = TOW1 + 4.0                         # string 2 ends two strings after string 1 began
MARK_ROWS = [2000 * j + 1999 - P0 for j in range(len(NUMBERS))]
FOUND_ROW = MARK_ROWS[-1]
# the runs of test_gpu_g1_if.py: a cut inside a symbol (rows 1000..1008 decide nothing), one row before the mark row of
# string 3, and one row after it
CHUNKS = (1004, MARK_ROWS[2] - 1 - 1004, 2, NPER - MARK_ROWS[2] - 1)

# name -> carrier phase rad.  The two phases give the two signs of the prompt sum the Costas loop can settle on; which
# phase gives which polarity is a property of the pull-in from this hand-over state, stated by POLARITY as the oracle
# shows it (test_g1_if_host.py asserts it there, before a GPU sees the signal).
CASES = {"phase0.7": 0.7, "phase3.84": 3.84}
POLARITY = {"phase0.7": 1, "phase3.84": -1}


def sent():
    """(the 1400 symbols +-1 as transmitted, the 85 bits of each string)."""
    return gs.stream(NUMBERS, STRING_SEED, tk=TK, nt=NT, n4=N4, slot=SLOT, iode=IODE)


def predict_sync(symbols, cnt0=CNT0, p0=P0):
    """(row in which flagsync rises, synci) from the sent symbols alone: the 51st sign change at a symbol edge with
    cnt > 2000 (NAVSYNCTH = 50, ref src/sdr.h:157); p0: the code period of the recording that row 0 holds."""
    votes, e = 0, (-p0) % RATE                  # the first row that begins a symbol
    while True:
        if cnt0 + e > 2000 and symbols[(p0 + e) // RATE - 1] != symbols[(p0 + e) // RATE]:
            votes += 1
            if votes == 51:
                return e, ((cnt0 + e) % RATE - 1) % RATE
        e += RATE


def case(name):
    """dict(phase, cnt0, sent, bits, sync_row, synci, rows: log row in which each decided symbol closes, symi: the sent
    symbol each one is, polarity)."""
    symbols, bits = sent()
    sync_row, synci = predict_sync(symbols)
    rows = np.arange(sync_row + RATE - 1, NPER, RATE)
    c = dict(name=name, phase=CASES[name], cnt0=CNT0, sent=symbols, bits=bits, sync_row=sync_row, synci=synci, rows=rows,
             symi=(P0 + rows) // RATE, polarity=POLARITY[name])
    assert np.all((P0 + rows) % RATE == RATE - 1) and FOUND_ROW == rows[-1] == NPER - 1
    return c


def sat(c):
    return dict(prn=FREQNO, doppler=FOFFSET + DOPPLER, codephase=CODEPHASE, cn0=CN0, phase=c["phase"],
                bits=c["sent"].astype(np.float64), symbol_periods=RATE)


_SIGNALS = {}


def signal(gc, synth, name):
    """The recording of a case, generated once per process."""
    if name not in _SIGNALS:
        codes = {FREQNO: gc.gencode(FREQNO, CTYPE_G1)}
        _SIGNALS[name] = synth.make_if(codes, NSAMP * (NPER + 3), f_sf=F_SF, f_if=0.0, dtype=2, sats=[sat(case(name))],
                                       seed=SIGNAL_SEED, f_cf=NOCODEDOPPLER)
    return _SIGNALS[name]


def channel(gc, freqno=FREQNO, **kw):
    return gc.Channel(freqno, ctype=gc.CTYPE_G1, dtype=2, f_sf=F_SF, f_if=0.0, **TAPS, **kw)


def oracle_channel(orc, c):
    """The oracle's channel in the hand-over state of the case, and its buffloc."""
    import ctypes as C
    o = orc.make_chan(FREQNO, ctype=CTYPE_G1, dtype=2, f_sf=F_SF, f_if=0.0, **TAPS)
    assert (o.rate, o.loopms, o.nsamp, o.foffset) == (RATE, 10, NSAMP, FOFFSET)
    o.acq.acqfreq = ACQFREQ
    o.carrfreq, o.codefreq, o.remcode, o.remcarr = ACQFREQ, o.crate, 0.0, 0.0
    o.flagsync, o.synci, o.cnt = 0, 0, c["cnt0"]
    return o, C.c_uint64(B0)


_ORACLE = {}


def oracle_run(gc, orc, synth, name):
    """The oracle's closed loop over the recording, free-running, once per process: dict(flagsync, navbit, buffloc, I:
    [NPER] columns of its rows, synci, carrfreq)."""
    import ctypes as C
    if name not in _ORACLE:
        c = case(name)
        sig = signal(gc, synth, name)
        ring = orc.make_ring(sig, sig.shape[0], sig.shape[0])
        o, b = oracle_channel(orc, c)
        L = orc.lib()
        fs, nb, loc, I = (np.zeros(NPER, t) for t in (np.int32, np.int32, np.uint64, np.float64))
        for e in range(NPER):
            loc[e] = b.value
            assert L.orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(b)) == 1
            fs[e], nb[e], I[e] = o.flagsync, (o.bit if (o.flagsync and o.swsync) else 0), o.II[0]
        _ORACLE[name] = dict(flagsync=fs, navbit=nb, buffloc=loc, I=I, synci=int(o.synci), carrfreq=float(o.carrfreq))
    return _ORACLE[name]


_REPLAYS = {}


def replayed(navbit, buffloc, cnt0=CNT0):
    """G1Replay after the rows of one run, computed once per process for equal inputs."""
    key = (np.asarray(navbit, np.int32).tobytes(), np.asarray(buffloc, np.uint64).tobytes(), cnt0)
    if key not in _REPLAYS:
        _REPLAYS[key] = gr.G1Replay().run_log(navbit, buffloc, cnt0)
    return _REPLAYS[key]
