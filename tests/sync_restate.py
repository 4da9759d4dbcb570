"""A literal Python restatement of gnsscorr_sync_* (include/gnsscorr.h): the body of the
reference's syncthread() loop (ref src/sdrsync.c:49-121) with interp1() and uint64todouble() (ref src/sdrcmn.c:505-565)
over per-channel histories of 80 rows, and the deterministic order in which pushed rows are consumed.  The tests'
reference for every output field, bit for bit: Python floats are IEEE doubles and every expression keeps the C code's
operations and their order; sample counts are Python integers masked to 64 bits (not a conftest)."""
import math

NH, PTIMING, CLIGHT, WEEKSEC, QCAP = 80, 68.802, 299792458.0, 3600 * 24 * 7, 4096
M64 = (1 << 64) - 1
ROW_FIELDS = ("tow", "remcout", "L", "D", "S", "codei", "cntout", "snr")
OUT_FIELDS = ("ch", "week", "tow", "P", "L", "D", "S", "sampref")


def u2d(v):
    """(double) of a uint64: Python's int -> float rounds to nearest even, as the conversion instruction does."""
    return float(v & M64)


def toint64(v):
    """double -> int64 towards zero as x86-64 does it (what does not fit gives 0x8000000000000000), as a uint64."""
    if not (-9223372036854775808.0 < v < 9223372036854775808.0):
        return 1 << 63
    return int(v) & M64


def crem(a, b):
    """C's a % b for b > 0: the sign of the dividend."""
    return a - b * (abs(a) // b) * (1 if a >= 0 else -1)


def interp1(x, y, t):
    n = len(x)
    if x[0] > x[n - 1]:
        xx, yy = x[::-1], y[::-1]
    else:
        xx, yy = list(x), list(y)
    if t <= xx[1]:
        k, m = 0, 2
    elif t >= xx[n - 2]:
        k, m = n - 3, n - 1
    else:
        k, m = 1, n
        while m - k != 1:
            i = (k + m) // 2
            if t < xx[i - 1]:
                m = i
            else:
                k = i
        k, m = k - 1, m - 1
        if abs(t - xx[k]) < abs(t - xx[m]):
            k -= 1
        else:
            m += 1
    assert 0 <= k and m <= n - 1
    z = 0.0
    for i in range(k, m + 1):
        s = 1.0
        for j in range(k, m + 1):
            if j != i:
                s = fdiv(s * (t - xx[j]), xx[i] - xx[j])
        z = z + s * yy[i]
    return z


def fdiv(a, b):
    """IEEE division, zero divisors included."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


class Chan:
    def __init__(self, nsamp, ctime, ti):
        self.nsamp, self.ctime, self.ti = nsamp, ctime, ti
        self.clear()

    def clear(self):
        self.attached = self.eligible = False
        self.tow, self.remcout, self.L, self.D = ([0.0] * NH for _ in range(4))
        self.codei, self.cntout = [0] * NH, [0] * NH
        self.S0, self.week, self.firstsf, self.firstsfcnt = 0.0, 0, 0, 0
        self.q, self.last = [], None


class SyncRestate:
    """push(ch, frame, rows): frame = dict(flagdec, week, firstsf, firstsfcnt), rows = dicts of ROW_FIELDS.  Epoch rows
    collect in .out as tuples in the order of OUT_FIELDS.  Refusals raise ValueError (EINVAL) / RuntimeError (ESTATE)."""

    def __init__(self, nch, outms):
        if nch <= 0 or outms <= 0:
            raise ValueError("create")
        self.nch, self.outms = nch, outms
        self.chan = [None] * nch
        self.ind = [0] * nch
        self.reftow = 0.0
        self.out = []

    def channel(self, ch, nsamp, ctime, ti):
        ok = lambda v: 0 < v < math.inf
        if not 0 <= ch < self.nch or nsamp <= 0 or not ok(ctime) or not ok(ti):
            raise ValueError("channel")
        if any(c is not None and c.ti != ti for i, c in enumerate(self.chan) if i != ch):
            raise ValueError("ti")
        self.chan[ch] = Chan(nsamp, ctime, ti)
        self.chan[ch].attached = True

    def push(self, ch, frame, rows):
        if not 0 <= ch < self.nch or self.chan[ch] is None:
            raise ValueError("push")
        c = self.chan[ch]
        last = c.last
        for r in rows:
            if last is not None and r["codei"] <= last:
                raise ValueError("codei")
            last = r["codei"]
        if not rows:
            return
        if len(c.q) + len(rows) > QCAP:
            raise RuntimeError("cap")
        c.q += [(r, frame) for r in rows]
        c.last, c.attached = last, True
        self.drain(False)

    def detach(self, ch):
        if not 0 <= ch < self.nch:
            raise ValueError("detach")
        if self.chan[ch] is not None:
            self.chan[ch].clear()
        self.drain(False)

    def flush(self):
        self.drain(True)

    def drain(self, everything):
        while True:
            att = [(i, c) for i, c in enumerate(self.chan) if c is not None and c.attached]
            waiting = [(c.q[0][0]["codei"], i) for i, c in att if c.q]
            if not waiting or (not everything and len(waiting) < len(att)):
                return
            self.consume(min(waiting)[1])

    def consume(self, ch):
        c = self.chan[ch]
        r, fr = c.q.pop(0)
        for name in ("tow", "remcout", "L", "D", "codei", "cntout"):
            h = getattr(c, name)
            h.pop()
            h.insert(0, r[name])
        if r["snr"]:
            c.S0 = r["S"]
        c.week, c.firstsf, c.firstsfcnt = fr["week"], fr["firstsf"], fr["firstsfcnt"]
        c.eligible = bool(fr["flagdec"]) and fr["week"] != 0 and r["cntout"] >= fr["firstsfcnt"]
        self.poll()

    def poll(self):
        isat = [i for i, c in enumerate(self.chan) if c is not None and c.eligible]
        nsat = len(isat)
        oldreftow, reftow = self.reftow, float(WEEKSEC)
        for i in isat:
            if self.chan[i].tow[0] < reftow:
                reftow = self.chan[i].tow[0]
        self.reftow = reftow
        if nsat == 0 or oldreftow == reftow:
            return
        ms = reftow * 1000
        if not ms > -2147483649.0:
            return
        if crem(int(ms), self.outms) != 0:
            return
        ind = self.ind
        for p, i in enumerate(isat):
            tow = self.chan[i].tow
            for j in range(NH):
                if abs(tow[j] - reftow) < 1E-4:
                    ind[p] = j
                    break
        mincodei, refi = M64, 0
        for p, i in enumerate(isat):
            if self.chan[i].codei[ind[p]] < mincodei:
                refi, mincodei = p, self.chan[i].codei[ind[p]]
        r = self.chan[isat[refi]]
        diffcnt = (r.cntout[ind[refi]] - r.firstsfcnt) & M64
        sampref = (r.firstsf + toint64(r.nsamp * (-PTIMING / (1000 * r.ctime) + u2d(diffcnt)))) & M64
        sampbase = (r.codei[NH - 1] - 10 * r.nsamp) & M64
        samprefd = u2d(sampref - sampbase)
        for p, i in enumerate(isat):
            c = self.chan[i]
            P = CLIGHT * c.ti * (u2d(c.codei[ind[p]] - sampref) - c.remcout[ind[p]])
            codeid = [u2d(v - sampbase) for v in c.codei]
            self.out.append((i, c.week, reftow + PTIMING / 1000, P, interp1(codeid, c.L, samprefd),
                             interp1(codeid, c.D, samprefd), c.S0, sampref))


def rows_of(arr):
    """numpy array of ObsRow -> list of dicts with Python scalars."""
    return [dict((n, (int if n in ("codei", "cntout", "snr") else float)(r[n])) for n in ROW_FIELDS) for r in arr]


def out_of(arr):
    """numpy array of EpochObs -> list of tuples in the order of OUT_FIELDS."""
    return [tuple((int if n in ("ch", "week", "sampref") else float)(r[n]) for n in OUT_FIELDS) for r in arr]


def same_bits(a, b):
    """Two lists of epoch rows equal bit for bit (-0.0 differs from 0.0); a NaN equals any NaN: the sign and payload of
    one that an operation makes are the processor's choice, not IEEE's."""
    import struct
    pack = lambda rows: [tuple(("nan" if v != v else struct.pack("<d", v)) if isinstance(v, float) else v for v in r)
                         for r in rows]
    return pack(a) == pack(b)
