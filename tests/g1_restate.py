"""A literal Python restatement of gnsscorr_g1frame_replay (include/gnsscorr.h): what the
reference's sdrnavigation() does behind checkbit() for CTYPE_G1 (ref src/sdrnav.c:40-82, src/sdrnav_glo.c), the time
functions included (RTKLIB's epoch2time / utc2gpst / time2gpst on whole seconds).  The tests' reference for every state
field; plain Python integers throughout (not a conftest)."""
import numpy as np

FLEN, PRELEN, UPDATE, EPHCNT = 200, 30, 2000, 5
# the ICD's time mark, first symbol first; a one is sent, and held here, as -1
MARK_BITS = "111110001101110101000010010110"
MARK = [-1 if c == "1" else 1 for c in MARK_BITS]
INT_FIELDS = ("polarity", "flagsyncf", "flagtow", "flagdec", "id", "ephcnt", "s1cnt", "nt", "slot", "n4", "iode", "update",
              "week", "firstsf", "firstsfcnt")
DBL_FIELDS = ("firstsftow", "tow_gpst")

LEAPS = [(2017, 1, 18), (2015, 7, 17), (2012, 7, 16), (2009, 1, 15), (2006, 1, 14), (1999, 1, 13), (1997, 7, 12),
         (1996, 1, 11), (1994, 7, 10), (1993, 7, 9), (1992, 7, 8), (1991, 1, 7), (1990, 1, 6), (1988, 1, 5), (1985, 7, 4),
         (1983, 7, 3), (1982, 7, 2), (1981, 7, 1)]
DOY = [1, 32, 60, 91, 121, 152, 182, 213, 244, 274, 305, 335]
DOYL = [1, 32, 61, 92, 122, 153, 183, 214, 245, 275, 306, 336]


def cdiv(a, b):
    """C's integer division: towards zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def epoch2time(year, mon, day, h=0, m=0, s=0):
    """Seconds since 1970-01-01; 0 outside 1970..2099 / months 1..12.  The day enters linearly."""
    if year < 1970 or year > 2099 or mon < 1 or mon > 12:
        return 0
    days = (year - 1970) * 365 + cdiv(year - 1969, 4) + DOY[mon - 1] + day - 2 + (1 if year % 4 == 0 and mon >= 3 else 0)
    return days * 86400 + h * 3600 + m * 60 + s


def utc2gpst(t):
    for y, m, leap in LEAPS:
        if t >= epoch2time(y, m, 1):
            return t + leap
    return t


def glo_date(nt, n4):
    """(year, month, day) as glot2time() derives them, quirks and all."""
    j = doy = day = 0
    if nt <= 366:
        j, doy = 1, nt
    elif nt <= 731:
        j, doy = 2, nt - 366 + 1
    elif nt <= 1096:
        j, doy = 3, nt - 731 + 1
    elif nt <= 1461:
        j, doy = 4, nt - 1096 + 1
    year = 1996 + 4 * (n4 - 1) + (j - 1)
    tab = DOYL if j == 1 else DOY
    mon = 12                                    # the value the loop variable is left with when nothing breaks
    for k in range(1, 12):
        if doy < tab[k]:
            day = doy - tab[k - 1]
            mon = k
            break
    return year, mon, day


def glot2time(nt, n4, tk):
    year, mon, day = glo_date(nt, n4)
    return utc2gpst(epoch2time(year, mon, day, tk[0], tk[1], tk[2]))


def time2gpst(t):
    """(week, seconds of week) since 1980-01-06."""
    sec = t - epoch2time(1980, 1, 6)
    w = cdiv(sec, 86400 * 7)
    return w, sec - w * 86400 * 7


def getbitu(buff, pos, n):
    v = 0
    for i in range(pos, pos + n):
        v = (v << 1) | ((buff[i >> 3] >> (7 - (i & 7))) & 1)
    return v


class G1Replay:
    """State as gnsscorr_g1frame_t; run() is the replay over decided symbols."""

    def __init__(self):
        self.fbits = [0] * FLEN
        for f in INT_FIELDS:
            setattr(self, f, 0)
        self.tk = [0, 0, 0]
        self.str = bytes(11)
        self.firstsftow = self.tow_gpst = 0.0
        self.marks = []                         # (cnt, polarity) of every time mark found: for the tests, not a state field

    def decode(self):
        b1 = [(self.polarity if i % 2 == 0 else -self.polarity) * self.fbits[i] for i in range(170)]
        b2 = [-1] + [b1[2 * i] * b1[2 * (i + 1)] for i in range(84)]
        buf = bytearray(11)
        for i, b in enumerate(b2):
            if b < 0:
                buf[i >> 3] |= 0x80 >> (i & 7)
        self.str = bytes(buf)
        self.id = getbitu(buf, 1, 4)
        if self.id == 1:
            self.tk = [getbitu(buf, 9, 5) - 3, getbitu(buf, 14, 6), 30 * getbitu(buf, 20, 1)]
        elif self.id == 2:
            iode = getbitu(buf, 9, 7)
            if iode != self.iode:
                self.update = 1
            self.iode = iode
        elif self.id == 4:
            self.nt, self.slot = getbitu(buf, 59, 11), getbitu(buf, 70, 5)
        elif self.id == 5:
            self.n4 = getbitu(buf, 49, 5)
        if 1 <= self.id <= 5:
            self.ephcnt += 1
        self.s1cnt = 1 if self.id == 1 else self.s1cnt + 1
        if self.ephcnt == EPHCNT:
            self.week, tow = time2gpst(glot2time(self.nt, self.n4, self.tk))
            self.tow_gpst = float(tow) + self.s1cnt * 2.0

    def run(self, symbols, cnts, bufflocs):
        """symbols[k]: the log's nonzero navbit at sdrthread's cnt cnts[k] and sample bufflocs[k]."""
        for bit, cnt, loc in zip(symbols, cnts, bufflocs):
            bit, cnt, loc = int(bit), int(cnt), int(loc)
            assert bit in (1, -1)
            self.fbits = self.fbits[1:] + [bit]
            if not self.flagtow:
                corr = sum(a * b for a, b in zip(self.fbits[FLEN - PRELEN:], MARK))
                self.flagsyncf = int(abs(corr) == PRELEN)
                if self.flagsyncf:
                    self.polarity = 1 if corr > 0 else -1
                    self.firstsf, self.firstsfcnt, self.flagtow = loc, cnt, 1
                    self.marks.append((cnt, self.polarity))
            if self.flagtow and (cnt - self.firstsfcnt) % UPDATE == 0:
                # ((int)(cnt - firstsfcnt) % 2000 in C: cnt >= firstsfcnt here, so the signs agree)
                self.decode()
                if self.tow_gpst == 0:
                    self.flagsyncf = self.flagtow = 0
                elif cnt == self.firstsfcnt:
                    self.flagdec = 1
                    self.firstsftow = self.tow_gpst
        return self

    def run_log(self, navbit, buffloc, cnt0):
        rows = np.flatnonzero(navbit)
        return self.run(np.asarray(navbit)[rows], cnt0 + rows, np.asarray(buffloc)[rows])

    def fields(self):
        d = {f: int(getattr(self, f)) for f in INT_FIELDS}
        d.update({f: float(getattr(self, f)) for f in DBL_FIELDS})
        d.update(tk=[int(v) for v in self.tk], str=bytes(self.str), fbits=[int(v) for v in self.fbits])
        return d


def state_fields(st):
    """The same dict of a G1FrameState (ctypes)."""
    d = {f: int(getattr(st, f)) for f in INT_FIELDS}
    d.update({f: float(getattr(st, f)) for f in DBL_FIELDS})
    d.update(tk=list(st.tk), str=bytes(st.str), fbits=list(st.fbits))
    return d
