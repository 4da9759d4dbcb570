"""GLONASS G1 navigation strings for the tests, built from fields (GLONASS ICD 5.1, sections 3.3.2 and 4; not a
conftest): 85 bits per string, first sent first -- position p here is the ICD's bit 85 - p, the numbering getbitu() of
the reference reads (ref src/sdrnav_glo.c): position 0 the idle bit (0), 1..4 the string number, 5..76 data, 77..84
the Hamming check bits.  Neither the reference nor this library reads the check bits, so they are filled at random like
every other position no field covers -- these are not valid ICD strings to a receiver that checks the code.

On the air a string is 2 s: the 85 bits in relative code (c[0] = 0, c[i] = c[i-1] xor bit[i]), each for 20 ms under the
100 Hz meander (the symbol, then its complement: two 10 ms symbols), then the 30-symbol time mark.  A one is sent as -1."""
import numpy as np

import g1_restate as gr

NBITS, NSYM = 85, 200


def _put(bits, pos, n, value):
    assert 0 <= value < (1 << n), (pos, n, value)
    for i in range(n):
        bits[pos + i] = (value >> (n - 1 - i)) & 1


def string_bits(number, rng, tk=None, iode=None, nt=None, slot=None, n4=None):
    """The 85 bits of string `number` (0..15).  tk = (hours of Moscow time 0..23, minutes, 0 / 1 half minutes) goes into
    string 1, iode (the ICD's t_b, 7 bits) into string 2, nt and slot into string 4, n4 into string 5; everything else,
    the Hamming check bits included, is random."""
    bits = rng.integers(0, 2, size=NBITS).astype(np.int64)
    bits[0] = 0
    _put(bits, 1, 4, number)
    if number == 1 and tk is not None:
        _put(bits, 9, 5, tk[0]); _put(bits, 14, 6, tk[1]); _put(bits, 20, 1, tk[2])
    if number == 2 and iode is not None:
        _put(bits, 9, 7, iode)
    if number == 4:
        if nt is not None:
            _put(bits, 59, 11, nt)
        if slot is not None:
            _put(bits, 70, 5, slot)
    if number == 5 and n4 is not None:
        _put(bits, 49, 5, n4)
    return bits


def string_symbols(bits):
    """The 200 symbols (+-1) of one string: relative code, meander, time mark."""
    c = np.bitwise_xor.accumulate(np.asarray(bits, np.int64))
    v = 1 - 2 * c                               # a one is -1
    return np.concatenate([np.stack([v, -v], axis=1).ravel(), np.array(gr.MARK, np.int64)])


def stream(numbers, seed, polarity=1, **fields):
    """(symbols +-1 [200 * len(numbers)], the bits of each string) of the strings `numbers` in a row."""
    rng = np.random.default_rng(seed)
    bits = [string_bits(m, rng, **fields) for m in numbers]
    return polarity * np.concatenate([string_symbols(b) for b in bits]), bits


def packed(bits):
    """The 11 bytes decode_g1() packs a string into: its first bit forced to one (ref src/sdrnav_glo.c:214), the tail
    zero."""
    b = np.concatenate([[1], np.asarray(bits[1:], np.int64), np.zeros(3, np.int64)]).astype(np.uint8)
    return bytes(np.packbits(b))


def meandered_data(n, seed):
    """n symbols of meandered relative-coded random bits with no time mark among them."""
    rng = np.random.default_rng(seed)
    v = 1 - 2 * np.bitwise_xor.accumulate(rng.integers(0, 2, size=(n + 1) // 2))
    return np.stack([v, -v], axis=1).ravel()[:n]


def log_rows(gc, symbols, first_period=0, step=10, cnt0=0, nper=None):
    """A synthetic closed-loop log (numpy array of gc.TrkLog): symbol i decided in row first_period + step * i, every
    other row navbit 0, buffloc 1000 * cnt."""
    symbols = np.asarray(symbols)
    n = first_period + step * len(symbols) if nper is None else nper
    log = np.zeros(n, dtype=np.dtype(gc.TrkLog))
    log["navbit"][first_period + step * np.arange(len(symbols))] = symbols
    log["buffloc"] = 1000 * (cnt0 + np.arange(n, dtype=np.uint64))
    return log


# ---- the time a string carries, derived with datetime alone (independent of g1_restate's RTKLIB restatement) ----------
_LEAP_DATES = [((1999, 1, 1), 13), ((2006, 1, 1), 14), ((2009, 1, 1), 15), ((2012, 7, 1), 16), ((2015, 7, 1), 17), ((2017, 1, 1), 18)]


def glonass_day(year, month, day):
    """(nt, n4) of a calendar date: day number within the four-year interval that begins with a leap year (1 = its 1st
    of January), and the number of that interval (1 = 1996..1999)."""
    import datetime as dt
    first = year - (year - 1996) % 4
    return (dt.date(year, month, day) - dt.date(first, 1, 1)).days + 1, (first - 1996) // 4 + 1


def gps_week_tow(year, month, day, h, m, s):
    """(GPS week, seconds of week) of a Moscow-time instant: minus 3 h is UTC, plus the leap seconds of that UTC instant
    is GPS time, counted from 1980-01-06.  Valid from 1999 on."""
    import datetime as dt
    utc = dt.datetime(year, month, day, h, m, s) - dt.timedelta(hours=3)
    leap = max(n for d, n in _LEAP_DATES if utc >= dt.datetime(*d))
    sec = int((utc - dt.datetime(1980, 1, 6)).total_seconds()) + leap
    return sec // 604800, sec % 604800
