"""The lock monitor at rate 2 inside the receiver schedule: the scenario of tests/test_lock_host.py (on the oracle alone:
what it decides, and the thresholds) and tests/test_gpu_rx_lock_sbas.py (on the device).  Not a conftest.

One ring of int8 IQ at 4.092 Msps, 7 s pushed in chunks of 0.25 s with one scheduling step each, three channels from
SEARCH:
  PRN 120  SBAS, symbols tied to the code epoch (synth.make_if, symbol_periods 2), four messages behind LEAD symbols,
           switched off at T_OFF, about 1 s after its frame.  Its code phase (1663.7 chips) puts the two rows checksync
           looks at first, cnt 2001 and 2002, into one symbol: the right edge, whatever was sent.
  PRN 133  SBAS, the same stream of symbols one code period out of step (code phase 311.3 chips): the same two rows
           straddle two symbols that were sent alike, so the first hand-over finds the wrong edge
           (tests/sbas_if_cases.py).  Always on.
  PRN 12   L1 C/A with 50 bit/s data, always on: the monitor's launch holds two bit lengths.

Geometry: a hand-over at sample b starts row 0 (cnt 0) at code period P = round((codephase + rate*b/f_sf) / 1023) of the
absolute code phase; row e holds code period P + e of symbol (P + e) // 2; sbas_if_cases.predict_sync gives the row in
which the edge is found and which edge it is.

Thresholds at rate 2: the detector's whole range is 1 (noise) to 2.  The window means below were
measured on the CPU oracle by tests/test_lock_host.py::test_rate2_thresholds_and_scenario_on_the_oracle, which asserts
them; MU_MIN sits midway between the smallest locked mean and the largest mean on noise or on the wrong edge."""
import numpy as np

import fec_restate as fr
import lock_cases as lc
import sbas_if_cases as sic

F_SF, NSAMP, CHUNK = lc.F_SF, lc.NSAMP, lc.CHUNK
DURATION = 7.0
NCHUNK = int(DURATION / 0.25)
MAX_PERIODS = lc.MAX_PERIODS
RETRY_MS = lc.RETRY_MS
CN0 = 47.0
SEED = 733
TAPS = lc.TAPS
# (prn, ctype, rate, Doppler Hz, code phase chips)
CHANNELS = [(120, lc.CTYPE_SBAS, 2, 2210.0, 640.7 + 1023.0), (133, lc.CTYPE_SBAS, 2, -1240.0, 311.3),
            (12, lc.CTYPE_L1CA, 20, -3222.0, 12.8)]
PRNS = [c[0] for c in CHANNELS]
RATES = [c[2] for c in CHANNELS]
LEAD = 1135                                      # message 0 starts a few symbols behind the symbol synchronisation
NSYM = 3600                                      # 7.2 s of symbols: LEAD of junk, four messages, junk
T_OFF = 6.3
TOW, WEEK = sic.TOW, sic.WEEK
STREAM_SEED = 22                                 # (lead symbols 1120 and 1121 alike: PRN 133's first hand-over straddles them)

KBITS, NBAD = 50, 2
# measured on the oracle (see the module docstring), window means of KBITS symbols
MU_LOCKED_MIN = 1.95                             # locked on the right edge (PRN 120 while on, PRN 133's second run), smallest; rounded down
MU_OTHER_MAX = 1.22                              # noise after T_OFF and PRN 133 on the wrong edge, largest; rounded up
MU_MIN = 0.5 * (MU_LOCKED_MIN + MU_OTHER_MAX)
PRM_SBAS = dict(sync_periods=2600, kbits=KBITS, nbad=NBAD, mu_min=MU_MIN)
PRM_WATCH = dict(PRM_SBAS, nbad=10 ** 6)         # the detector watching only: every window mean, no loss by reason 2
PRM = [PRM_SBAS, PRM_SBAS, lc.PRM]


def symbols():
    """The +-1 symbols both SBAS satellites send: symbol s while the absolute code phase is in [2046 s, 2046 (s+1))."""
    s = fr.sbas_stream(sic.messages(), 1, LEAD, seed=STREAM_SEED)
    rng = np.random.default_rng(STREAM_SEED + 1)
    tail = (1 - 2 * rng.integers(0, 2, size=NSYM - len(s))).astype(np.int8)
    return np.concatenate([s, tail])


def sats():
    rng = np.random.default_rng(SEED)
    sym = symbols().astype(np.float64)
    out = []
    for i, (prn, ctype, rate, dop, cph) in enumerate(CHANNELS):
        d = dict(prn=prn, doppler=dop, codephase=cph, cn0=CN0, phase=0.7 + 0.4 * i)
        if ctype == lc.CTYPE_SBAS:
            d.update(bits=sym, symbol_periods=2)
        else:
            d.update(bits=rng.choice([-1.0, 1.0], size=64))
        out.append(d)
    out[0]["t_off"] = T_OFF
    return out


def signal(gc, synth):
    codes = {p: gc.gencode(p, ct) for p, ct, _, _, _ in CHANNELS}
    return synth.make_if(codes, NCHUNK * CHUNK, f_sf=F_SF, f_if=0.0, dtype=2, sats=sats(), seed=SEED)


def channels(gc):
    return [gc.Channel(p, ctype=ct, dtype=2, f_sf=F_SF, f_if=0.0, **TAPS) for p, ct, _, _, _ in CHANNELS]


def step_wrpos():
    return [CHUNK * (k + 1) for k in range(NCHUNK)]


def code_period(i, buffloc):
    """The code period of the absolute code phase that starts at the hand-over sample `buffloc` of channel i."""
    _, _, _, dop, cph = CHANNELS[i]
    rate = 1.023e6 * (1.0 + dop / 1575.42e6)
    x = (cph + rate * buffloc / F_SF) / 1023.0
    assert abs(x - round(x)) < 0.01, x           # the hand-over is on a code epoch to a few hundredths of a period
    return int(round(x))


def predict(i, buffloc):
    """(sync row = cnt, synci, right edge?, cnt of the frame or None) of a hand-over of SBAS channel i at `buffloc`."""
    p = code_period(i, buffloc)
    row, synci, right = sic.predict_sync(symbols(), 0, p0=p)
    found = 2 * (LEAD + 1511) + 1 - p
    return row, synci, right, (found if right and (p + row) // 2 <= LEAD else None)


def oracle_schedule(gc, orc, sig, i, prm=None, keep_rows=False):
    prn, ctype, rate, _, _ = CHANNELS[i]
    return lc.oracle_schedule(gc, orc, sig, prn, PRM[i] if prm is None else prm, ctype=ctype, rate=rate, taps=TAPS,
                              wrpos=step_wrpos(), keep_rows=keep_rows)
