"""Scenarios of the drop-in symbols at other sample rates than 16.368 Msps and at long periods (helpers of
tests/test_gpu_symbols_rates.py, which runs them on the device, and of tests/test_symbol_rate_cases.py, which shows on
the oracle alone that each is what it claims; not a conftest).

A ring does not know a sample rate: initsdrch()'s f_sf gives a struct its nsamp, so channels of different rates read
the same ring and the oracle is given the same f_sf.  The tracking scenarios (A) therefore need no satellite at the
claimed rate -- the bar is equality with the oracle, bit for bit -- and run on two rings of uniform random int8
samples, ring 1 real and ring 2 IQ, NBLK blocks each.  The acquisition scenarios (B) need one, and get a short
synthetic recording per rate.

Segment counts are period_edge_cases.nseg / first_nsamp / front_end (the restatement of gc_trk_nseg the batched tests
use); nothing of it is repeated here.
"""
import numpy as np

import acq_cases as ac
import period_edge_cases as pe
import symbol_cases as sc

BLK = sc.BLK
# three periods of 262144 samples and sdrtracking()'s `bufflocnow > buffloc` margin of one more nsamp behind a start
# below START_MAX: two consecutive periods of the longest length, 14 blocks
NBLK = 14
WRPOS = NBLK * BLK
START_MAX = 4000
RING_SEEDS = (41, 42)
_cache = {}


def ring_samples():
    """(int8 [n], int8 [n, 2]): full-scale uniform noise, the two rings of the tracking scenarios."""
    if "rings" not in _cache:
        _cache["rings"] = (np.random.default_rng(RING_SEEDS[0]).integers(-128, 128, size=WRPOS, dtype=np.int8),
                           np.random.default_rng(RING_SEEDS[1]).integers(-128, 128, size=(WRPOS, 2), dtype=np.int8))
    return _cache["rings"]


def queue_nseg(dtype, n):
    """Segments of a launch chain of sdrtracking()'s queue whose longest request has n samples.  An engine sizes its
    segments for nsamp + 100 samples (the longest period the reference tracks), which is what period_edge_cases.nseg
    states; the queue sizes each chain for the group's longest currnsamp itself (cmb_run_group: gc_trk_nseg(dtype,
    max_n)), so its counts change 100 samples later."""
    return pe.nseg(dtype, n - 100)


def rate_chan(key, ring, taps, prn, nsamp):
    """A channel on ring 1 (real) or 2 (IQ) whose 1 ms code periods have nsamp samples."""
    f_sf, f_if = pe.front_end(nsamp, ring)
    c = sc.chan(key, ring, taps, prn, f_sf=f_sf, f_if=f_if)
    c["nsamp"] = nsamp
    return c


def periods(nsamp, cap):
    """Periods a channel of this length can track from a start below START_MAX: the oracle and the library both want
    one more nsamp behind a period's first sample."""
    return min(cap, (WRPOS - START_MAX) // (nsamp + 100) - 1)


def start(c, salt=0):
    """(acqfreq, buffloc of the first period): a bin of the 200 Hz grid and an unaligned position, reproducible."""
    rng = np.random.default_rng([c["prn"], c["ring"], c["nsamp"], salt])
    return sc.ringcfg(c)["f_if"] + 200.0 * int(rng.integers(-20, 21)), int(rng.integers(0, START_MAX))


def hand_over(x, c, salt=0, state=None):
    """Library struct or oracle channel x at c's start state; state = (remcode, Doppler Hz) replaces what an
    acquisition leaves: the code phase, and the carrier and (by the same ratio as dll()'s carrier aiding) code
    frequency of that Doppler.  Returns buffloc."""
    acqfreq, b = start(c, salt)
    sc.hand_over(x, acqfreq, x.crate)
    if state is not None:
        t = x.trk if hasattr(x, "trk") else x
        x.acq.acqfreq = t.carrfreq = sc.ringcfg(c)["f_if"] + state[1]
        t.remcode, t.codefreq = state[0], x.crate + state[1] / (sc.F_CF / x.crate)
    return b


def oracle_rows(orc, c, nper, salt=0, state=None):
    """The oracle's rows (symbol_cases.oracle_track) of c from its start state: once per process."""
    key = ("rows", c["key"], nper, salt, state)
    if key not in _cache:
        o = sc.oracle_chan(orc, c)
        assert o.nsamp == c["nsamp"], (c["key"], o.nsamp)
        b = hand_over(o, c, salt, state)
        ring = ring_samples()[c["ring"] - 1]
        rows, _ = sc.oracle_track(orc, o, orc.make_ring(ring, sc.RINGLEN, WRPOS), b, nper)
        assert max(r[0][0] for r in rows) <= c["nsamp"] + 100       # (the reference's scratch: nsamp + 100 samples)
        _cache[key] = rows
    return _cache[key]


# ---- A.1: one thread, one struct per length, in this order ---------------------------------------------------------
def seq_lengths(dtype):
    """16368 (one segment), the first length of three segments, 65536 (no edge table), 262144 (eleven segments), 2048,
    16368 again: the queue's buffers grow twice, then serve one segment from buffers sized for eleven."""
    return [16368, pe.first_nsamp(dtype, 3), 65536, pe.NSAMP_MAX, 2048, 16368]


SEQ_NSEG = [1, 3, 3, 11, 1, 1]           # pe.nseg of seq_lengths (asserted on the host): what an engine would use
SEQ_QUEUE_NSEG = [1, 2, 3, 11, 1, 1]     # queue_nseg: what the queue launches with; its capacity grows three times
SEQ_CAP = 3


def seq(ring):
    return [rate_chan("q%d_%d_%d" % (ring, i, n), ring, "A", 1 + i + 8 * (ring - 1), n)
            for i, n in enumerate(seq_lengths(ring))]


# ---- A.2: periods on both sides of the first segment boundary -------------------------------------------------------
# nsamp == first_nsamp(dtype, 2), where an engine's segment count changes, and nsamp == first_nsamp(dtype, 2) + 100,
# where the queue's does (queue_nseg); (code phase, Doppler) below: dll() sets the code frequency anew every period as chip
# rate - codeNco + Doppler / 1540, so an offset of the code frequency alone is gone after one period, while a Doppler of
# 21 kHz keeps the code a third of a sample per period fast through the carrier aiding: currnsamp alternates between
# first_nsamp - 1 (one segment) and first_nsamp (two) while the filters, fed with noise, move both frequencies by a few
# Hz a period.  Found on the host with the oracle (a sweep of 20 .. 45 kHz: both rings alternate every period from
# this one); that both values occur, one behind the other, is held by tests/test_symbol_rate_cases.py.
BOUNDARY_NPER = 6
BOUNDARY_STATE = {1: (0.0105, 21000.0), 2: (0.0105, 21000.0)}


BOUNDARIES = ("engine", "queue")


def boundary(ring, which):
    n = pe.first_nsamp(ring, 2) + (100 if which == "queue" else 0)
    return rate_chan("edge%d_%s" % (ring, which), ring, "A", 17 + ring, n)


# ---- A.3: short beside long in one group, threaded ------------------------------------------------------------------
MIXED_CAP = 12                            # periods of the short members; the longest has two


def mixed(ring):
    """One (dtype, corrn 2) group of 2048, 16368, first_nsamp(3) and 262144 samples, tap sets A (smax 6) and B (smax 16)
    of each, and four members of corrn 6 (tap set C) at 16368 and 65536: a batch splits into two groups of other nseg."""
    out, prn = [], 1
    for n in (2048, 16368, pe.first_nsamp(ring, 3), pe.NSAMP_MAX):
        for t in "AB":
            out.append(rate_chan("m%d_%d%s" % (ring, n, t), ring, t, prn, n))
            prn += 1
    for n in (16368, 65536):
        for j in range(2):
            out.append(rate_chan("m%d_%dC%d" % (ring, n, j), ring, "C", prn, n))
            prn += 1
    return out


def mixed_nper(c):
    return periods(c["nsamp"], MIXED_CAP)


# a 2048-sample and a 262144-sample request in one launch chain, known by counting: a 262144-sample request of corrn 6
# goes first and keeps the leader busy; the pair (corrn 2) queues up behind it
PAIR_TRIES = 6


def pair(ring, k):
    """(blocker, short, long) of attempt k."""
    return (rate_chan("pb%d_%d" % (ring, k), ring, "C", 25, pe.NSAMP_MAX),
            rate_chan("ps%d_%d" % (ring, k), ring, "A", 26, 2048),
            rate_chan("pl%d_%d" % (ring, k), ring, "B", 27, pe.NSAMP_MAX))


# ---- A.4: after the mixed batches, one thread again: A.1's structs of 262144 and of 2048 samples -------------------
def after(ring):
    s = seq(ring)
    return [s[3], s[4]]


# ---- B: sdracquisition() at the transform lengths -------------------------------------------------------------------
# rate: f_sf, dtype (its ring), f_if, nsamp, the satellite (48 dB-Hz or more: the first window decides), blocks pushed
ACQ_GRID = (400, 200)                     # five bins, set on the struct after initsdrch() (intg stays 10)
RATES = {
    "rtlsdr_2048": dict(f_sf=2.048e6, dtype=2, f_if=0.0, nsamp=2048, prn=4, doppler=190.0, cn0=50.0, seed=2048),
    "gn3s_8183": dict(f_sf=8.1838e6, dtype=1, f_if=38.4e3, nsamp=8183, prn=6, doppler=-210.0, cn0=50.0, seed=8183),
    "fft32k_16384": dict(f_sf=16.384e6, dtype=2, f_if=0.0, nsamp=16384, prn=10, doppler=390.0, cn0=50.0, seed=16384),
    "fft64k_16385": dict(f_sf=16.385e6, dtype=1, f_if=16.385e6 / 4, nsamp=16385, prn=12, doppler=-20.0, cn0=50.0, seed=16385),
    "longest_32768": dict(f_sf=32.768e6, dtype=2, f_if=0.0, nsamp=32768, prn=15, doppler=-380.0, cn0=50.0, seed=32768),
}
ACQ_INTG = 10                             # ACQINTG_L1CA
ACQ_NPER = 6                              # periods tracked behind the hand-over
ABSENT = ("rtlsdr_2048", 22)             # (every window acq_cases.MARGIN from a tie: PRN 20 has one at 4e-4)
REFUSED_NSAMP = 65536                     # a 65.536 Msps struct: the search is refused, tracking is not
REFUSED_NPER = 3
REINIT = ("fft32k_16384", "rtlsdr_2048")  # one struct address across rates: both IQ, the same ring re-created


def acq_blocks(name):
    """Blocks pushed before the search: (intg + 1) * nsamp samples look-back and a little more."""
    return -(-((ACQ_INTG + 1) * RATES[name]["nsamp"] + 1000) // BLK)


def acq_chan(name, prn=None):
    r = RATES[name]
    c = sc.chan(name, r["dtype"], "A", r["prn"] if prn is None else prn, f_sf=r["f_sf"], f_if=r["f_if"])
    c["nsamp"] = r["nsamp"]
    return c


def acq_recording(gc, synth, name):
    """The rate's recording: its satellite's code periods start a third of a period into the first search window, half
    a sample into the chip (acq_cases.sat_at)."""
    key = ("rec", name)
    if key not in _cache:
        r, n = RATES[name], RATES[name]["nsamp"]
        total = acq_blocks(name) * BLK
        s_ref = total - (ACQ_INTG + 1) * n + n // 3 + n            # (in the second period of the first window)
        sat = ac.sat_at(r["prn"], s_ref % n, n, r["f_sf"], r["doppler"], r["cn0"], phase=0.7, mid=s_ref // n, into=0.5)
        codes = {r["prn"]: gc.gencode(r["prn"], sc.CTYPE_L1CA)}
        _cache[key] = synth.make_if(codes, total, f_sf=r["f_sf"], f_if=r["f_if"], dtype=r["dtype"], sats=[sat], seed=r["seed"])
    return _cache[key]


def cut_grid(x, c):
    """The five-bin Doppler grid on a library struct (acq.nfreq / acq.freq edited in place) or an oracle channel."""
    hband, step = ACQ_GRID
    if hasattr(x, "trk"):
        x.acq.nfreq = 2 * (hband // step) + 1
        for i in range(x.acq.nfreq):
            x.acq.freq[i] = x.f_if + (i - (x.acq.nfreq - 1) // 2) * float(step) + x.foffset
    else:
        ac.grid(x, hband, step, ACQ_INTG)
    return x


def oracle_search(orc, name, buf, prn=None):
    """(oracle channel after its search, symbol_cases.oracle_acq_full's dict) of the rate's channel over buf."""
    c = acq_chan(name, prn)
    o = cut_grid(sc.oracle_chan(orc, c), c)
    assert o.nsamp == c["nsamp"] and o.nfreq == 5
    return o, sc.oracle_acq_full(orc, o, orc.make_ring(buf, sc.RINGLEN, len(buf)))


def power_floor(nsamp):
    return sc.POWER_FLOOR * nsamp / 16368
