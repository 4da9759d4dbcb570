"""numpy restatement of the SBAS L1 frame path (test infrastructure, like spec_restate.py): the K = 7, rate-1/2 Viterbi
decoder as DESIGN.md 3.5 defines it (libfec's portable viterbi27 as ref src/sdrnav.c:302-318 drives it), the matching
encoder, CRC-24Q, an SBAS message builder, and a plain replay of ref src/sdrnav.c:40-82 for CTYPE_L1SBAS on a list of
decided symbols.  Written from those definitions, not from the library's C.

The trellis loops run step by step as the definition states them; numpy carries the 64 states and, in front of them,
any number of independent windows (a batch axis: every window is decoded by the same loop, none sees another)."""
import numpy as np

POLYA, POLYB = 0x6d, 0x4f               # libfec's V27POLYA, V27POLYB (fec.h), in the order ref src/sdrinit.c:502 uses
WIN, NDEC, ROWBYTES = 1512, 750, 96     # NAVFLEN_SBAS + NAVADDFLEN_SBAS symbols; flen/2 bits; bytes of a packed row
UPDATE = 1000                           # ref src/sdrinit.c:530: flen/3*rate periods
PREAMBLES = (0x53, 0x9A, 0xC6)
# ref src/sdrinit.c:498-500, elements 0..15 as they stand
PREBITS = (1, -1, 1, -1, 1, 1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1)


def parity(x):
    x = np.asarray(x)
    p = np.zeros_like(x)
    for i in range(7):
        p ^= (x >> i) & 1
    return p


# ---- encoder / decoder ------------------------------------------------------------------------------------------
def encode(bits, polyA=POLYA, polyB=POLYB, state=0):
    """+-1 symbols (two per bit) of `bits` from encoder state `state` (the last six bits, newest in bit 0): a symbol
    is -1 where the parity of register & polynomial is one (received as 255), +1 where it is zero (received as 0)."""
    out = np.empty(2 * len(bits), np.int8)
    for n, b in enumerate(bits):
        r = (state << 1) | int(b)
        out[2 * n] = -1 if bin(r & polyA).count("1") & 1 else 1
        out[2 * n + 1] = -1 if bin(r & polyB).count("1") & 1 else 1
        state = r & 63
    return out


def viterbi27(fbits, ndec, polyA=POLYA, polyB=POLYB):
    """Decoded bits [..., ndec] (0 / 1) of the windows fbits[..., win] (+1, -1 or 0), win even."""
    f = np.asarray(fbits)
    win = f.shape[-1]
    assert win % 2 == 0 and 0 <= ndec <= win // 2 - 6
    nstep = win // 2
    rx = np.where(f == 1, 0, 255).astype(np.int32)        # (756*510 + 63 fits with room to spare)
    s = np.arange(64, dtype=np.int32)
    b = s & 1
    p0, p1 = s >> 1, (s >> 1) + 32                  # the two states that reach s; p0 < 32
    r0, r1 = (p0 << 1) | b, (p1 << 1) | b
    eA0, eB0 = 255 * parity(r0 & polyA), 255 * parity(r0 & polyB)
    eA1, eB1 = 255 * parity(r1 & polyA), 255 * parity(r1 & polyB)
    metric = np.broadcast_to(np.where(s == 0, 0, 63).astype(np.int32), f.shape[:-1] + (64,))
    words = np.zeros(f.shape[:-1] + (nstep,), np.uint64)
    for t in range(nstep):
        ra, rb = rx[..., 2 * t, None], rx[..., 2 * t + 1, None]
        m0 = metric[..., p0] + (eA0 ^ ra) + (eB0 ^ rb)
        m1 = metric[..., p1] + (eA1 ^ ra) + (eB1 ^ rb)
        d = m1 < m0                                  # the smaller sum survives; equal sums keep p0
        metric = np.where(d, m1, m0)
        words[..., t] = np.packbits(d, axis=-1, bitorder="little").view("<u8")[..., 0]
    assert metric.max() < 2 ** 32                    # uint32 in the definition, never renormalised
    state = np.zeros(f.shape[:-1], np.uint64)
    bits = np.zeros(f.shape[:-1] + (nstep,), np.uint8)
    for t in range(nstep - 1, -1, -1):               # from state 0, whatever the metrics say
        bits[..., t] = state & np.uint64(1)
        d = (words[..., t] >> state) & np.uint64(1)
        state = (state >> np.uint64(1)) | (d << np.uint64(5))
    return bits[..., :ndec]


def pack_rows(bits, rowbytes):
    """MSB first, zero padded to rowbytes, as gnsscorr_fec_run writes them."""
    p = np.packbits(np.asarray(bits, np.uint8), axis=-1)
    out = np.zeros(p.shape[:-1] + (rowbytes,), np.uint8)
    out[..., :p.shape[-1]] = p
    return out


def windows(stream, pos0, npos, stride, win):
    """[npos][win]: window p ends at symbol pos0 + p*stride of the stream; symbols in front of it are 0."""
    s = np.concatenate([np.zeros(win, np.int8), np.asarray(stream, np.int8)])
    ends = win + pos0 + stride * np.arange(npos)
    return s[(ends - (win - 1))[:, None] + np.arange(win)[None, :]]


def fec_rows(sym, pos0, npos, stride=1, win=WIN, ndec=NDEC, polyA=POLYA, polyB=POLYB, rowbytes=None, chunk=512):
    """What gnsscorr_fec_run returns for sym[nch][nsym] (or [nsym]): uint8 [nch][npos][rowbytes]."""
    sym = np.atleast_2d(np.asarray(sym, np.int8))
    rowbytes = (ndec + 7) // 8 if rowbytes is None else rowbytes
    out = np.zeros((sym.shape[0], npos, rowbytes), np.uint8)
    for c in range(sym.shape[0]):
        w = windows(sym[c], pos0, npos, stride, win)
        for i in range(0, npos, chunk):
            out[c, i:i + chunk] = pack_rows(viterbi27(w[i:i + chunk], ndec, polyA, polyB), rowbytes)
    return out


# ---- CRC-24Q and the message builder ----------------------------------------------------------------------------
CRC24Q_POLY = 0x1864CFB


def crc24q(bits):
    """Remainder of bits * x^24 by the polynomial, as long division on one integer; leading zeros do not count."""
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    v <<= 24
    while v.bit_length() > 24:
        v ^= CRC24Q_POLY << (v.bit_length() - 25)
    return v


def _bits(value, n):
    return [(value >> (n - 1 - i)) & 1 for i in range(n)]


def sbas_message(index, mtype, body=None, tow=None, week=None):
    """250 bits: preamble PREAMBLES[index % 3], the 6-bit type, 212 data bits, CRC-24Q over those 226.  Type 12 with
    tow / week carries them where ref src/sdrnav_sbs.c:69-73 reads them: bits 107..126 = tow - 1, 127..136 = week - 1024."""
    body = [0] * 212 if body is None else [int(b) for b in body]
    assert len(body) == 212
    m = _bits(PREAMBLES[index % 3], 8) + _bits(mtype, 6) + body
    if tow is not None:
        m[107:127] = _bits(int(tow) - 1, 20)
        m[127:137] = _bits(int(week) - 1024, 10)
    return m + _bits(crc24q(m), 24)


def sbas_stream(messages, polarity=1, lead=0, seed=0):
    """The messages encoded back to back from state 0 as +-1 symbols times polarity, behind `lead` random symbols."""
    bits = [b for m in messages for b in m]
    rng = np.random.default_rng(seed)
    junk = (1 - 2 * rng.integers(0, 2, size=lead)).astype(np.int8)
    return np.concatenate([junk, (polarity * encode(bits)).astype(np.int8)])


# ---- replay of ref src/sdrnav.c:40-82 for CTYPE_L1SBAS ----------------------------------------------------------
FIELDS = ("flagsyncf", "polarity", "flagtow", "flagdec", "flagpol", "firstsf", "firstsfcnt", "firstsftow", "tow_gpst",
          "week", "id")


class SbasReplay:
    """sdrnavigation() behind checkbit() on decided symbols: state as the reference's sdrnav_t / sdrsbas_t fields."""

    def __init__(self):
        self.fbits = np.zeros(WIN, np.int8)
        self.flagsyncf = self.polarity = self.flagtow = self.flagdec = self.flagpol = 0
        self.firstsf = self.firstsfcnt = 0
        self.firstsftow = self.tow_gpst = self.tow = 0.0
        self.week = self.id = 0
        self.msg = bytes(32)
        self.ndecodes = 0

    def run(self, symbols, cnts, bufflocs, aid_tow=None, aid_week=0, chunk=512):
        """symbols[k]: what checkbit() decided with flagpol off (the log's navbit), at sdrthread's cnt cnts[k] and
        sample bufflocs[k]; aid_tow[k]: the aiding channel's tow[0] at that period."""
        n = len(symbols)
        stream = np.concatenate([self.fbits, np.asarray(symbols, np.int8) * (-1 if self.flagpol else 1)])
        rows, lo, hi = None, 0, 0

        def predecodefec(k):
            nonlocal rows, lo, hi
            if not lo <= k < hi:                     # decode ahead while every symbol wants one
                lo, hi = k, (min(n, k + chunk) if not self.flagtow else k + 1)
                rows = viterbi27(windows(stream, WIN + lo, hi - lo, 1, WIN), NDEC)
                self.ndecodes += hi - lo
            return 1 - 2 * rows[k - lo].astype(np.int64)        # fbitsdec[0..749]: bit 0 -> +1, bit 1 -> -1

        for k in range(n):
            cnt = int(cnts[k])
            pos = WIN + k                            # checkbit() has appended the symbol: the window ends here
            if not self.flagtow:
                dec = predecodefec(pos - WIN)
                # findpreamble(): ref :384-389, :398-408
                corr = sum(int(dec[i]) * PREBITS[i] + int(dec[250 + i]) * PREBITS[8 + i] for i in range(8))
                self.flagsyncf = 0
                if abs(corr) == 16:
                    self.polarity = 1 if corr > 0 else -1
                    if self._paritycheck(dec):
                        self.flagsyncf = 1
                    elif self.polarity == 1 and not self.flagpol:
                        self.flagpol = 1             # checkbit() flips every symbol it decides from now on
                        stream[pos + 1:] *= -1
                        hi = min(hi, k + 1)
                if self.flagsyncf:
                    self.firstsf, self.firstsfcnt, self.flagtow = int(bufflocs[k]), cnt, 1
            if self.flagtow and (cnt - self.firstsfcnt) % UPDATE == 0:
                dec = predecodefec(pos - WIN)
                self._decode_l1sbas(dec, None if aid_tow is None else aid_tow[k], aid_week)
                if self.tow_gpst == 0:
                    self.flagsyncf = self.flagtow = 0
                elif cnt == self.firstsfcnt:
                    self.flagdec, self.firstsftow = 1, self.tow_gpst
        self.fbits = stream[n:].copy()

    def _message(self, dec):
        return [1 if self.polarity * int(v) < 0 else 0 for v in dec[:250]]

    def _paritycheck(self, dec):
        m = self._message(dec)
        return crc24q(m[:226]) == int("".join(map(str, m[226:250])), 2)

    def _decode_l1sbas(self, dec, aid_tow, aid_week):
        m = self._message(dec)
        self.msg = bytes(np.packbits(np.array(m + [0] * 6, np.uint8)))
        self.id = int("".join(map(str, m[8:14])), 2)
        if self.id == 12:
            self.tow = int("".join(map(str, m[107:127])), 2) + 1.0
            self.week = int("".join(map(str, m[127:137])), 2) + 1024
        else:
            self.tow += 1.0
        if aid_tow is not None and aid_week != 0:
            self.tow, self.week = float(aid_tow), int(aid_week)
        if self.week != 0:
            self.tow_gpst = self.tow

    def fields(self):
        return {f: getattr(self, f) for f in FIELDS} | {"msg": self.msg}


def log_columns(symbols, first_period=0, cnt0=0, step=2):
    """A synthetic closed-loop log for the symbols: symbol i decided in period first_period + step*i (rate 2), buffloc
    1000 * cnt.  Returns (navbit[nper], buffloc[nper], cnts[nsym], bufflocs[nsym])."""
    n = len(symbols)
    nper = first_period + step * n
    navbit = np.zeros(nper, np.int32)
    per = first_period + step * np.arange(n)
    navbit[per] = symbols
    buffloc = 1000 * (cnt0 + np.arange(nper, dtype=np.uint64))
    return navbit, buffloc, cnt0 + per, buffloc[per]
