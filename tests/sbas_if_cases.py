"""SBAS L1 signals that carry symbols (synth.make_if with symbol_periods = 2) and what the receiver must find in them
(tests/test_sbas_if_host.py holds the CPU oracle to it, tests/test_gpu_sbas_if.py the device; not a conftest): PRN 120 on
int8 IQ at 4.092 Msps, four messages behind a few lead symbols, tracked from the acquisition hand-over state with cnt
preset just below 2000.

Geometry.  The generator's symbol s lasts while the absolute code phase codephase + rate*t lies in [2046 s, 2046 (s+1)):
code periods 2s and 2s + 1.  The tracker starts at the first code epoch of the recording, code period P0 = 1 (code phase
100.2 chips), so log row e holds code period P0 + e of symbol (P0 + e) // 2, at sdrthread's cnt = cnt0 + e.  checksync's
rate-2 shift register looks at rows with cnt > 2000 and synchronises on the first two consecutive rows of equal sign,
synci = cnt % 2 of the second; checkbit then decides a symbol in every row with cnt % 2 == synci, from that row's and
the previous row's prompt sum.  If the synchronising row is the second period of a symbol (P0 + e odd) every decided
symbol is one sent symbol -- the right edge; if it is the first, every decision adds the second half of one symbol and
the first half of the next -- the wrong edge: where the two differ the decision is made on noise, and no frame is found.
Which of the two happens is decided by the parity of cnt0 and by the sent symbols around cnt 2001 alone.

The frame: the reference finds message 0 (preamble 0x53, followed by 0x9A) when its window of 1512 symbols ends at the
message's last symbol with the tail, symbol lead + 1511, i.e. in row 2 (lead + 1511) + 1 - P0."""
import numpy as np

import fec_restate as fr
from test_fec_host import spaced_errors

F_SF, NSAMP = 4.092e6, 4092
PRN, CTYPE_SBAS = 120, 27
DOPPLER, CODEPHASE, CN0 = -830.0, 100.2, 47.0
TAPS = dict(corrn=2, corrd=1, corrp=1)
RATE = 2
P0 = int(CODEPHASE // 1023) + 1                 # the code period of log row 0
B0 = int(round((1023 - CODEPHASE % 1023) * 4)) % NSAMP
ACQFREQ = 200.0 * round(DOPPLER / 200.0)
TOW, WEEK = 345600, 1900
LEAD = 7
NMSG = 4
NSYM = LEAD + 500 * NMSG                        # sent symbols
NPER = 2 * NSYM - P0                            # rows 0 .. NPER-1: the last one closes the last sent symbol
SIGNAL_SEED = 120
# the runs of test_gpu_sbas_if.py: a call of one period before and one after the symbol edge is found, a cut between the
# two periods of a symbol (before row 1500 and before row 1501: one of them whatever the edge), and a cut right before
# the row of firstsfcnt
FOUND_ROW = 2 * (LEAD + 1511) + 1 - P0
CHUNKS = (1, 12, 1487, 1, FOUND_ROW - 1501, NPER - FOUND_ROW)


def messages(seed=31):
    """Four messages; message 0 is type 12 with TOW / WEEK."""
    rng = np.random.default_rng(seed)
    types = [12, 2, 25, 4]
    return [fr.sbas_message(i, types[i], rng.integers(0, 2, size=212), tow=TOW if i == 0 else None, week=WEEK)
            for i in range(NMSG)]


def flip_positions():
    """Sent-symbol indices flipped in the flip case: spaced as test_fec_host.spaced_errors, inside message 0's window."""
    return LEAD + spaced_errors(2)


# name -> (carrier phase rad, cnt0, flips).  The two phases give the two signs of the prompt sum the Costas loop can
# settle on; which phase gives which polarity is a property of the pull-in from this hand-over state, stated by
# POLARITY below as the oracle shows it (test_sbas_if_host.py asserts it there, before a GPU sees the signal).
CASES = {
    "right_phase0.7": (0.7, 1990, False),
    "right_phase3.84": (3.84, 1990, False),
    "wrong_edge": (0.7, 1991, False),
    "right_flips": (0.7, 1990, True),
}
POLARITY = {"right_phase0.7": -1, "right_phase3.84": 1, "wrong_edge": None, "right_flips": -1}


def sent_symbols(flips=False):
    """(+-1 symbols as transmitted, the same without the flips)."""
    clean = fr.sbas_stream(messages(), 1, LEAD, seed=3)
    assert len(clean) == NSYM
    sent = clean.copy()
    if flips:
        idx = flip_positions()
        sent[idx] = -sent[idx]
    return sent, clean


def predict_sync(sent, cnt0, p0=P0):
    """(row in which flagsync rises, synci, right edge?) from the sent symbols alone: the first row with cnt > 2001 whose
    sign equals the previous row's (the register holds a zero until its second entry)."""
    e = max(2001 - cnt0, 0) + 1
    while sent[(p0 + e - 1) // 2] != sent[(p0 + e) // 2]:
        e += 1
    return e, (cnt0 + e) % 2, (p0 + e) % 2 == 1


def case(name):
    """dict(phase, cnt0, sent, clean, flips, sync_row, synci, right, rows: log row in which each decided symbol closes,
    cnts: sdrthread's cnt of those rows, symi: the sent symbol each one is (right edge) or ends in (wrong edge),
    firstsfcnt / found_row: where the frame must be found (None: never), msg: message 0 packed as the replay holds it,
    polarity)."""
    phase, cnt0, flips = CASES[name]
    sent, clean = sent_symbols(flips)
    sync_row, synci, right = predict_sync(sent, cnt0)
    rows = np.arange(sync_row, NPER, 2)
    c = dict(name=name, phase=phase, cnt0=cnt0, sent=sent, clean=clean, flips=flip_positions() if flips else np.zeros(0, np.int64),
             sync_row=sync_row, synci=synci, right=right, rows=rows, cnts=cnt0 + rows, symi=(P0 + rows) // 2,
             polarity=POLARITY[name], firstsfcnt=None, found_row=None,
             msg=bytes(np.packbits(np.array(messages()[0] + [0] * 6, np.uint8))))
    if right:
        c["found_row"] = FOUND_ROW
        c["firstsfcnt"] = cnt0 + FOUND_ROW
        assert (P0 + FOUND_ROW) // 2 == LEAD + 1511 and FOUND_ROW in rows and c["symi"][0] <= LEAD
    return c


def sat(c):
    return dict(prn=PRN, doppler=DOPPLER, codephase=CODEPHASE, cn0=CN0, phase=c["phase"], bits=c["sent"].astype(np.float64),
                symbol_periods=RATE)


_SIGNALS = {}


def signal(gc, synth, name):
    """The recording of a case, generated once per process (cases that differ only in cnt0 share it)."""
    c = case(name)
    key = (c["phase"], bool(len(c["flips"])))
    if key not in _SIGNALS:
        codes = {PRN: gc.gencode(PRN, CTYPE_SBAS)}
        _SIGNALS[key] = synth.make_if(codes, NSAMP * (NPER + 3), f_sf=F_SF, f_if=0.0, dtype=2, sats=[sat(c)], seed=SIGNAL_SEED)
    return _SIGNALS[key]


def oracle_channel(orc, c):
    """The oracle's channel in the hand-over state of the case, and its buffloc."""
    import ctypes as C
    o = orc.make_chan(PRN, ctype=CTYPE_SBAS, dtype=2, f_sf=F_SF, f_if=0.0, **TAPS)
    assert (o.rate, o.loopms, o.nsamp) == (RATE, 2, NSAMP)
    o.acq.acqfreq = ACQFREQ
    o.carrfreq, o.codefreq, o.remcode, o.remcarr = ACQFREQ, o.crate, 0.0, 0.0
    o.flagsync, o.synci, o.cnt = 0, 0, c["cnt0"]
    return o, C.c_uint64(B0)


_REPLAYS = {}


def replayed(symbols, cnts, bufflocs):
    """SbasReplay after these decided symbols (one run), computed once per process for equal inputs."""
    key = (np.asarray(symbols, np.int8).tobytes(), np.asarray(cnts, np.int64).tobytes(), np.asarray(bufflocs, np.uint64).tobytes())
    if key not in _REPLAYS:
        rep = fr.SbasReplay()
        rep.run(np.asarray(symbols, np.int8), np.asarray(cnts, np.int64), np.asarray(bufflocs, np.uint64))
        _REPLAYS[key] = rep
    return _REPLAYS[key]
