"""Synthetic SBAS L1 symbol streams for the frame-synchronisation tests (test_fec_host.py on the restatement alone,
test_gpu_sbasframe.py against the device): built with fec_restate's message builder and encoder.

The reference synchronises on a message that starts with 0x53 and is followed by one that starts with 0x9A, i.e. on
message 0, 3, 6, ... of a stream; the window of 1512 symbols holds such a message first once its 1512th symbol is
in, so message m is found at symbol lead + 500*m + 1511."""
import numpy as np

import fec_restate as fr

TOW, WEEK = 345600, 1900
AID_WEEK = 1901


def _bodies(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 2, size=212) for _ in range(n)]


def basic_messages(seed=11, time=True):
    """Five messages; the first is type 12 with TOW / WEEK (time) or type 3 (no time anywhere)."""
    b = _bodies(5, seed)
    types = [12 if time else 3, 2, 25, 4, 63]
    return [fr.sbas_message(i, types[i], b[i], tow=TOW if (time and i == 0) else None, week=WEEK) for i in range(5)]


def flagpol_messages(seed=12, j=20):
    """Ten messages, none with time before message 6 (type 12).  Message 0 is found and dropped again (no time), then
    bits j..j+7 of message 0 read 0x53 and those of message 1 read 0x9A: a preamble pair of polarity +1 whose CRC
    fails, j bits = 2j symbols later.  That raises flagpol; every later symbol is flipped, and the first message of
    index 0 mod 3 that lies wholly behind the flip is message 6, found with polarity -1."""
    b = _bodies(10, seed)
    b[0][j - 14:j - 6] = fr._bits(0x53, 8)          # data bit i is message bit 14 + i
    b[1][j - 14:j - 6] = fr._bits(0x9A, 8)
    types = [3, 2, 25, 4, 63, 9, 12, 2, 3, 4]
    return [fr.sbas_message(i, types[i], b[i], tow=TOW if i == 6 else None, week=WEEK) for i in range(10)]


def cases():
    """name -> dict(symbols, found: symbol index the frame is found at for good (None: never), polarity, flagpol,
    aid: use the aiding time)"""
    basic, notime, fp = basic_messages(), basic_messages(time=False), flagpol_messages()
    c = {}
    for pol in (1, -1):
        for lead in (0, 7):
            c["pol%+d_lead%d" % (pol, lead)] = dict(symbols=fr.sbas_stream(basic, pol, lead, seed=lead), found=lead + 1511,
                                                    polarity=pol, flagpol=0, aid=False)
    c["flagpol"] = dict(symbols=fr.sbas_stream(fp, 1, 3, seed=5), found=3 + 500 * 6 + 1511, polarity=-1, flagpol=1, aid=False)
    rng = np.random.default_rng(77)
    c["noframe"] = dict(symbols=(1 - 2 * rng.integers(0, 2, size=1700)).astype(np.int8), found=None, polarity=None,
                        flagpol=0, aid=False)
    c["aid"] = dict(symbols=fr.sbas_stream(notime, 1, 4, seed=6), found=4 + 1511, polarity=1, flagpol=0, aid=True)
    c["noaid"] = dict(symbols=fr.sbas_stream(notime, 1, 4, seed=6), found=None, polarity=1, flagpol=0, aid=False)
    return c


def aid_tow(nper, cnt0=0):
    """The aiding channel's tow[0] per period: 1 ms steps from 100000 s."""
    return 100000.0 + 0.001 * (cnt0 + np.arange(nper))


_REPLAYED = {}


def replayed(name, first_period=5, cnt0=0):
    """(case, SbasReplay after the whole stream, log columns), computed once per process."""
    key = (name, first_period, cnt0)
    if key not in _REPLAYED:
        case = cases()[name]
        navbit, buffloc, cnts, locs = fr.log_columns(case["symbols"], first_period, cnt0)
        rep = fr.SbasReplay()
        aid = aid_tow(len(navbit), cnt0) if case["aid"] else None
        rep.run(case["symbols"], cnts, locs, None if aid is None else aid[cnts - cnt0], AID_WEEK if case["aid"] else 0)
        _REPLAYED[key] = (case, rep, (navbit, buffloc, cnts, locs, aid))
    return _REPLAYED[key]
