"""Scenarios of the drop-in symbol tests (helpers of tests/test_gpu_symbols_receiver.py, which runs them on the device,
and of tests/test_symbol_cases.py, which shows on the oracle alone that each of them is decided with room; not a
conftest).

One receiver, RX2, serves most of them: the file front end with both IF streams, ring 1 real samples at a 4.092 MHz
IF and ring 2 int8 IQ at zero IF, both at 16.368 Msps.  Its two files are one continuous synthetic recording each;
the tests consume them block by block (FILE_BUFFSIZE samples) in a fixed order:

    blocks 0..7     tracking from low positions (mixed groups, a refused request, re-initialised structs, > 256 structs)
    blocks 8..13    the ring's first wrap: they land at ring blocks 4996..4999, 0, 1
    blocks 14..19   the same at the 14th wrap, where the sample count has passed 2^32

A position in a file (`fpos`, samples from the file's start) and the absolute sample count the receiver knows it by
differ by a constant per stretch; the oracle only ever sees samples, so the host check runs on the files as they are.
"""
import ctypes as C

import numpy as np

F_SF = 16.368e6
NSAMP = 16368
BLK = 65536                       # FILE_BUFFSIZE
MEMBUFFLEN = 5000
RINGLEN = MEMBUFFLEN * BLK
F_CF = 1575.42e6
IF1 = dict(dtype=1, f_if=4.092e6)             # ring 1
IF2 = dict(dtype=2, f_if=0.0)                 # ring 2
LOOPB = dict(dllb=(5.0, 1.0), pllb=(30.0, 10.0), fllb=(200.0, 50.0))
TAPS = {"A": (2, 3, 3), "B": (2, 8, 8), "C": (6, 3, 6)}       # trkcorrn, trkcorrd, trkcorrp
CTYPE_L1CA, CTYPE_G1 = 1, 20
SYS_GPS, SYS_GLO = 1, 4
G1KEY = 100                       # the GLONASS code's key in the synthesiser's code table (frequency number 0)
# the existing closed-loop test's floor for the prompt power of a tracked satellite (tests/test_gpu_symbols.py)
POWER_FLOOR = 100 * (8.0 ** 2) * 16368 / 32 ** 2
MARGIN = 1e-3

NB_LOW, NB_WRAP = 8, 6
NBLOCKS = NB_LOW + 2 * NB_WRAP
WRAP_LAPS = (1, 14)               # 14 * RINGLEN = 4 587 520 000 > 2^32
WRAP_BEFORE = 4                   # blocks pushed before the ring's end; NB_WRAP - WRAP_BEFORE after it

# satellites of the two recordings (prn, Doppler Hz, code phase chips at sample 0, C/N0, carrier phase)
SATS1 = [dict(prn=1, doppler=1210.0, codephase=100.3, cn0=48.0, phase=0.3),
         dict(prn=3, doppler=-2790.0, codephase=640.8, cn0=48.0, phase=1.3),
         dict(prn=5, doppler=3405.0, codephase=901.1, cn0=48.0, phase=2.1),
         dict(prn=7, doppler=-400.0, codephase=333.3, cn0=41.0, phase=0.9)]       # weak: decided after the first window
SATS2 = [dict(prn=9, doppler=-1605.0, codephase=200.6, cn0=48.0, phase=0.5),
         dict(prn=11, doppler=2595.0, codephase=777.7, cn0=48.0, phase=2.5),
         dict(prn=G1KEY, doppler=810.0, codephase=123.4, cn0=48.0, phase=1.7)]
SEED1, SEED2 = 31, 32
ABSENT1 = 20


def chan(key, ring, taps, prn, ctype=CTYPE_L1CA, f_sf=None, f_if=None):
    """A channel of the receiver; f_sf / f_if: its own sample rate and IF (tests/symbol_rate_cases.py: the ring does not
    know a rate, initsdrch()'s f_sf gives a struct its nsamp), by default the recordings'."""
    c = dict(key=key, ring=ring, taps=taps, prn=prn, ctype=ctype)
    if f_sf is not None:
        c["f_sf"] = f_sf
    if f_if is not None:
        c["f_if"] = f_if
    return c


# the mixed receiver: (dtype, corrn) groups of 6, 2, 6 and 3 members; taps A and B share corrn 2 and differ in smax
MIXED = ([chan("r1_p%d" % p, 1, t, p) for p, t in zip(range(1, 9), "AABBCCAB")] +
         [chan("r2_p%d" % p, 2, t, p) for p, t in zip(range(9, 15), "ABCABC")] +
         [chan("r2_g%d" % k, 2, t, k, CTYPE_G1) for k, t in zip((0, 1, -1), "ABC")])
MIXED_NPER = 24
# A group member keeps its own smax: (code phase, offset of the code frequency from the chip rate) at which the replica
# walk of a 6-sample outermost tap and that of a 16-sample one (coff - smax * ci, wrapped, then + ci per position)
# round to different sides of a chip edge at the sample the period starts on -- an integer code phase and a non-dyadic
# chip step, found with csrc/gnsscorr_nco.h on the host and held there by tests/test_symbol_cases.py.  Every period of
# the edge channels starts from one of them.
EDGE_STATES = [(686.0, 1.85), (694.0, -1.64), (824.0, -2.11), (655.0, 1.15), (496.0, -0.59), (334.0, -1.87), (68.0, 2.68),
               (399.0, -2.92), (71.0, -1.43), (669.0, -1.18), (457.0, 1.16), (465.0, 1.39), (216.0, 1.92), (8.0, 0.49),
               (4.0, 2.11), (754.0, -0.95), (238.0, 2.97), (570.0, 0.92), (546.0, 0.22), (105.0, 2.36), (330.0, -0.24),
               (404.0, 1.86), (822.0, -0.01), (978.0, -0.25)]
EDGE = ([chan("e_a%d" % p, 1, "A", p) for p in range(1, 9)] +          # smax 6 ...
        [chan("e_b%d" % p, 1, "B", p) for p in range(9, 17)])          # ... beside smax 16, one (dtype, corrn) group
# a refused request beside good ones: struct names ring 1 (real samples) but carries dtype 2, and the other way round
REFUSED_GOOD = [MIXED[i] for i in (0, 2, 4, 8, 9, 14)]
REFUSED_NPER = 8
# re-initialised structs: tracked as A, freed and set up again as B (same length), its code overwritten in place by C's,
# then freed and set up as a 511-chip GLONASS channel on the other ring
REINIT = [chan("a", 1, "A", 1), chan("b", 1, "A", 3), chan("c", 1, "A", 5), chan("g", 2, "A", 0, CTYPE_G1)]
REINIT_NPER = 6
# more structs than the combiner's code table keeps
MANY_FIRST, MANY_BATCH = 250, 12        # tracked one by one, then two threaded batches of known and new structs: 264
MANY_KNOWN = (4, 6)                     # known structs in the first and in the second batch
# acquisition, struct re-used: one ring; then after a second rcvinit_file() with another front end
ACQ_A, ACQ_B = 1, 3                     # both present on recording 1
ACQ_C = 9                               # present on recording 2 (IQ, zero IF)
ACQ_NBLOCKS = 4                         # pushed before the searches: 262144 >= 11 * 16368 samples
# ring wrap: searched on ring 1 with the write position two blocks past the ring's end
WRAP_ACQ = (1, 7, ABSENT1)              # strong (first window), weak (a window that straddles the end), absent (all)
WRAP_TRK = [MIXED[0], MIXED[4], MIXED[8], MIXED[14]]     # tracked across the end: both rings, taps A, C, A, A
WRAP_TRK_BACK = 3 * NSAMP + 77          # first period starts this far before the end
WRAP_NPER = 8


def ringcfg(c):
    cfg = IF1 if c["ring"] == 1 else IF2
    return dict(cfg, f_if=c["f_if"]) if "f_if" in c else cfg


def rate_of(c):
    return c.get("f_sf", F_SF)


def codes(gc):
    out = {s["prn"]: gc.gencode(s["prn"], CTYPE_L1CA) for s in SATS1 + SATS2 if s["prn"] != G1KEY}
    out[G1KEY] = gc.gencode(0, CTYPE_G1)
    return out


def recordings(gc, synth):
    """The two files' samples: (int8 [n], int8 [n, 2])."""
    n = NBLOCKS * BLK
    cd = codes(gc)
    return (synth.make_if(cd, n, f_sf=F_SF, sats=SATS1, seed=SEED1, **IF1),
            synth.make_if(cd, n, f_sf=F_SF, sats=SATS2, seed=SEED2, **IF2))


def sat_of(c):
    """The satellite a channel follows, or None."""
    if c["ctype"] == CTYPE_G1:
        return SATS2[2] if c["prn"] == 0 else None
    for s in (SATS1 if c["ring"] == 1 else SATS2):
        if s["prn"] == c["prn"] and s["cn0"] >= 45.0:
            return s
    return None


def start_state(c, fpos0, salt=0):
    """(acqfreq, file position of the first period) of channel c for tracking that begins at or after fpos0: a present
    satellite's code period start and its Doppler's bin of the 200 Hz grid, as an acquisition would hand over;
    anything reproducible for the others."""
    cfg = ringcfg(c)
    foffset = 0.5625e6 * c["prn"] if c["ctype"] == CTYPE_G1 else 0.0
    s = sat_of(c)
    if s is None:
        rng = np.random.default_rng([c["prn"] + 1000, c["ring"], salt])
        return cfg["f_if"] + foffset + 200.0 * int(rng.integers(-20, 21)), fpos0 + int(rng.integers(0, NSAMP))
    clen, crate = (511, 0.511e6) if c["ctype"] == CTYPE_G1 else (1023, 1.023e6)
    rate = crate * (1.0 + s["doppler"] / F_CF)
    first = (clen - s["codephase"]) * F_SF / rate               # the first period start, in samples
    per = clen * F_SF / rate
    k = int(np.ceil((fpos0 - first) / per))
    return cfg["f_if"] + foffset + 200.0 * round(s["doppler"] / 200.0), int(round(first + max(k, 0) * per))


def oracle_chan(orc, c):
    corrn, corrd, corrp = TAPS[c["taps"]]
    return orc.make_chan(c["prn"], ctype=c["ctype"], f_sf=rate_of(c), corrn=corrn, corrd=corrd, corrp=corrp, **ringcfg(c), **LOOPB)


def set_ini(gc, taps="A"):
    """The [TRACK] section initsdrch() reads from the global sdrini."""
    ini = gc.sdrini()
    ini.trkcorrn, ini.trkcorrd, ini.trkcorrp = TAPS[taps]
    for k, v in LOOPB.items():
        name = "trk" + k
        getattr(ini, name)[0], getattr(ini, name)[1] = v
    return ini


def init_sdr(gc, c, sdr=None, chno=1):
    """initsdrch() for channel c, on a new struct or on the one given."""
    set_ini(gc, c["taps"])
    sdr = gc.SdrCh() if sdr is None else sdr
    cfg = ringcfg(c)
    sys_ = SYS_GLO if c["ctype"] == CTYPE_G1 else SYS_GPS
    assert gc.lib().initsdrch(chno, sys_, c["prn"], c["ctype"], cfg["dtype"], c["ring"], F_CF, rate_of(c), cfg["f_if"], C.byref(sdr)) == 0
    return sdr


def hand_over(x, acqfreq, crate):
    """What sdracquisition() leaves for the tracking loop, on a library struct or an oracle channel."""
    x.flagacq = 1
    x.acq.acqfreq = acqfreq
    t = x.trk if hasattr(x, "trk") else x
    t.carrfreq, t.codefreq = acqfreq, crate


def row_of(x):
    """One period's results of a library struct or an oracle channel, comparable with ==."""
    t = x.trk if hasattr(x, "trk") else x
    ntap = 1 + 2 * t.corrn
    return (x.currnsamp, tuple(t.II[:ntap]), tuple(t.QQ[:ntap]), t.remcode, t.remcarr)


def oracle_track(orc, o, ring, buffloc, nper):
    """sdrthread()'s loop before bit sync on the oracle (ref src/sdrmain.c:264-276): rows = (row_of, carrfreq,
    codefreq after the filters) per period; returns (rows, next buffloc)."""
    O = orc.lib()
    rows = []
    for _ in range(nper):
        O.orc_sdrtracking(C.byref(o), C.byref(ring), buffloc)
        assert o.flagtrk == 1, "the oracle has not enough samples: a mistake of the scenario"
        r = row_of(o)
        O.orc_cumsumcorr(C.byref(o), 1)
        O.orc_pll(C.byref(o), 0, o.ctime)
        O.orc_dll(C.byref(o), 0, o.ctime)
        O.orc_clearcumsumcorr(C.byref(o))
        rows.append((r, o.carrfreq, o.codefreq))
        buffloc += o.currnsamp
    return rows, buffloc


def symbol_track(gc, sdr, buffloc, nper, cnt0=0):
    """The same loop on the library's symbols."""
    L = gc.lib()
    rows = []
    for k in range(nper):
        L.sdrtracking(C.byref(sdr), buffloc, cnt0 + k)
        assert sdr.flagtrk == 1, ("sdrtracking refused", sdr.prn, buffloc)
        r = row_of(sdr)
        L.cumsumcorr(C.byref(sdr.trk), 1)
        L.pll(C.byref(sdr), C.byref(sdr.trk.prm1), sdr.ctime)
        L.dll(C.byref(sdr), C.byref(sdr.trk.prm1), sdr.ctime)
        L.clearcumsumcorr(C.byref(sdr.trk))
        rows.append((r, sdr.trk.carrfreq, sdr.trk.codefreq))
        buffloc += sdr.currnsamp
    return rows, buffloc


def edge_track(track_one, x, buffloc, first):
    """Periods that each start from an EDGE_STATES entry (from index `first` on, all of them once): the code phase and
    code frequency are set, track_one(buffloc) runs one sdrtracking() on x (a library struct or an oracle channel),
    no loop filter.  Returns the rows."""
    t = x.trk if hasattr(x, "trk") else x
    rows = []
    for k in range(len(EDGE_STATES)):
        coff, dc = EDGE_STATES[(first + k) % len(EDGE_STATES)]
        t.remcode, t.codefreq = coff, x.crate + dc
        track_one(buffloc)
        assert x.flagtrk == 1
        rows.append(row_of(x))
        buffloc += x.currnsamp
    return rows


def prompt_power(rows):
    return [r[0][1][0] ** 2 + r[0][2][0] ** 2 for r in rows]


def oracle_acq_full(orc, o, ring):
    """One orc_sdracquisition(): dict(flagacq, iters, buffloc, acqcodei, freqi, acqfreq, cn0, peakr, power)."""
    xc = orc.codespectrum(o)
    o.xcode = xc.ctypes.data
    power = np.zeros(o.nfreq * o.nsamp)
    it = C.c_int()
    try:
        buffloc = orc.lib().orc_sdracquisition(C.byref(o), C.byref(ring), power.ctypes.data, C.byref(it))
    finally:
        o.xcode = None
    return dict(flagacq=o.flagacq, iters=it.value, buffloc=int(buffloc), acqcodei=o.acq.acqcodei, freqi=o.acq.freqi,
                acqfreq=o.acq.acqfreq, cn0=o.acq.cn0, peakr=o.acq.peakr, power=power)


def check_acq(sdr, buffloc, want, where=""):
    """A struct after sdracquisition() against oracle_acq_full(): integers and buffloc exact, peakr and cn0 to 1e-4."""
    assert (sdr.flagacq, int(buffloc)) == (want["flagacq"], want["buffloc"]), (where, sdr.flagacq, buffloc, want["flagacq"], want["buffloc"])
    got = (sdr.acq.acqcodei, sdr.acq.freqi, sdr.acq.acqfreq)
    assert got == (want["acqcodei"], want["freqi"], want["acqfreq"]), (where, got, want["acqcodei"], want["freqi"], want["acqfreq"])
    for k in ("peakr", "cn0"):
        a, b = getattr(sdr.acq, k), want[k]
        assert abs(a - b) <= 1e-4 * abs(b), (where, k, a, b)


def wrap_segment(lap):
    """(first file block, block count the receiver is at when that block is pushed) of the wrap stretch of `lap`."""
    i = WRAP_LAPS.index(lap)
    return NB_LOW + i * NB_WRAP, lap * MEMBUFFLEN - WRAP_BEFORE


def many_chan(i):
    """Struct i of the > 256: PRNs 1..32 on ring 1 in turn, taps A."""
    return chan("m%d" % i, 1, "A", 1 + i % 32)
