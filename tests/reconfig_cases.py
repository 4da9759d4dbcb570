"""Reconfiguration of a live context: the inputs, the channel sets and the observation sequences shared
by tests/test_reconfig_host.py (which shows on the oracle and the restatements alone that every search used here is
decided with room) and tests/test_gpu_reconfig.py (which runs them on the device).  Helpers; not a conftest.

The bar of the device tests is bit-for-bit equality of everything a caller can fetch between a *live* engine -- one that
ran a configuration A, had its results fetched and was then reconfigured to B -- and *fresh* engines that only ever saw B
on the same ring contents, one of them with every device buffer poisoned (gnsscorr_debug_poison) so that the yardstick
cannot lean on zeros.  `freeze` turns what the fetch calls return into nested tuples of bytes (NaNs and signed zeros
compare by their bits), `diff` names where two frozen observations part.

Inputs are those of tests/acq_fine_cases.py -- `iq4`, `real4`, `coh`, `m26` and the hand-over signal -- the search span
at the stream's origin with noise behind it for the trackers to run over, rings sized by acq_edge_cases.granule.
"""
import ctypes as C
import struct

import numpy as np

import acq_cases as ac
import acq_edge_cases as ec
import acq_fine_cases as fc

N4 = fc.N4
F4 = 4.092e6
POISON = 0xA5
TRK_PERIODS = 75            # periods of the iq4 / real4 streams: batches of 12 + 12 + 30 and a closed loop of 60 fit


# ---- bit-for-bit comparison ------------------------------------------------------------------------------------------
def freeze(x):
    """A fetched value as nested tuples of bytes, ints and strings."""
    if isinstance(x, np.ndarray):
        return ("nd", x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (C.Structure, C.Array)):
        return ("ct", bytes(x))
    if isinstance(x, float):
        return ("f8", struct.pack("<d", x))
    if isinstance(x, dict):
        return ("dict",) + tuple((k, freeze(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return ("seq",) + tuple(freeze(v) for v in x)
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    if isinstance(x, np.floating):
        return freeze(float(x))
    assert x is None or isinstance(x, (int, str, bytes)), type(x)
    return x


def diff(a, b, path="", out=None, cap=8):
    """Paths at which the observations a and b (as fetched, not frozen) differ; [] when they are bit for bit equal."""
    out = [] if out is None else out
    if len(out) >= cap:
        return out
    if isinstance(a, dict) and isinstance(b, dict) and sorted(a) == sorted(b):
        for k in sorted(a):
            diff(a[k], b[k], f"{path}.{k}", out, cap)
    elif isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b):
        for i, (x, y) in enumerate(zip(a, b)):
            diff(x, y, f"{path}[{i}]", out, cap)
    elif isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype:
        if freeze(a) != freeze(b):
            raw = [np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (x.dtype.itemsize,)) for x in (a, b)]
            bad = np.argwhere((raw[0] != raw[1]).any(axis=-1))
            out.append(f"{path}: {len(bad)} of {a.size} elements, first at {tuple(int(v) for v in bad[0])}")
    elif freeze(a) != freeze(b):
        out.append(f"{path}: {a!r:.80} != {b!r:.80}" if not isinstance(a, (np.ndarray, C.Structure)) else f"{path}: bytes differ")
    return out


def same(a, b, where=""):
    """Asserts bit-for-bit equality of two observations, naming where they part."""
    assert freeze(a) == freeze(b), (where, diff(a, b))


def differ(a, b, where=""):
    assert freeze(a) != freeze(b), (where, "the two configurations give the same bytes: the comparison is vacuous")


# ---- channels --------------------------------------------------------------------------------------------------------
# Tap spacing (samples) by tap pairs: the outermost tap stays within 6 samples, 1.5 chips at the four samples per chip of
# these inputs -- the reach of the shipped layout (18 samples at 16 per chip).
CORRD = {1: 3, 2: 3, 3: 2, 6: 1}


def chan(gc, sc, spec, corrn=2, nref=0):
    """A device Channel for entry `spec` = (prn, hband, step, intg, ncoh, estep) of scenario dict `sc`, with corrn tap
    pairs CORRD[corrn] samples apart (early / late: the innermost pair)."""
    prn, hband, step, intg, ncoh, estep = spec
    c = gc.Channel(prn, dtype=sc["dtype"], f_sf=sc["f_sf"], f_if=sc["f_if"], hband=hband, step=step, intg=intg,
                   ncoh=ncoh, estep=estep, nref=nref, corrn=corrn, corrd=CORRD[corrn], corrp=CORRD[corrn])
    c.corrd = CORRD[corrn]
    return c


G4 = (1400, 200, 10, 1, 0)          # iq4's grid: 15 bins of 200 Hz, ten iterations
ABSENT4 = 17                        # a PRN that is neither in iq4's span nor in its channel list
# channel sets on iq4's ring, as PRNs: the shrink and grow sequences go between a set of six and a set of two whose
# first channels are other satellites than the other set's (so that the two sets' results differ channel by channel)
IQ4_SIX_A, IQ4_TWO_B = [3, 8, 14, 22, 5, ABSENT4], [22, 14]
IQ4_TWO_A, IQ4_SIX_B = [3, 8], [22, 14, 5, 8, 3, ABSENT4]
IQ4_THREE = [14, 5, 22]             # the set of the ring re-create and in-flight sequences
M26_EXTRA = (7, 200, 200, 4, 1, 0)  # m26's second channel: an absent PRN on the satellite's grid
SEARCHED = ("iq4", "real4", "coh", "m26")      # the scenarios whose searches the device tests hold against the oracle


def iq4_set(gc, prns, corrn, nref=0):
    return [chan(gc, fc.SCEN["iq4"], (p,) + G4, corrn, nref) for p in prns]


def scen_set(gc, name, corrn=2, nref=0, plain=False):
    """The Channels of scen_specs(name); plain: without the coherent and bit-edge settings."""
    return [chan(gc, fc.SCEN[name], s[:4] + (1, 0) if plain else s, corrn, nref) for s in scen_specs(name)]


def present(name):
    return {t[0] for t in fc.SCEN[name]["sats"]}


def scen_specs(name):
    """The channel entries a scenario is run with here: its own, m26 with its second channel, iq4 with ABSENT4."""
    specs = list(fc.SCEN[name]["chans"])
    if name == "m26":
        specs.append(M26_EXTRA)
    if name == "iq4":
        specs.append((ABSENT4,) + G4)
    return specs


_cache = {}


def wants(gc, orc, synth, name, plain=False):
    """prn -> restated search result of scenario `name` with the span at the stream's origin and the search ending at
    the span's last sample, for every entry of scen_specs(name).  plain: the entries searched with ncoh 1 and estep 0
    (what a channel set is after gnsscorr_set_channels).  Computed once per process."""
    key = ("wants", name, plain)
    if key not in _cache:
        sc = fc.SCEN[name]
        W = fc.scenario(gc, orc, synth, name)[0]
        specs = scen_specs(name)
        if plain:
            specs = [s[:4] + (1, 0) for s in specs]
        pairs = [ec.pair(gc, orc, sc, s) for s in specs]
        _cache[key] = dict(zip([s[0] for s in specs], ec.restate(orc, pairs, W, len(W), len(W))))
    return _cache[key]


def stream(gc, orc, synth, name, periods=None):
    """The scenario's span followed by noise up to `periods` code periods (None: the span alone), and the ring length
    that holds it whole."""
    key = ("stream", name, periods)
    if key not in _cache:
        sc = fc.SCEN[name]
        W = fc.scenario(gc, orc, synth, name)[0]
        n = ec.cc.nsamp(sc)
        s = W if periods is None else np.concatenate([W, ac.noise(periods * n - len(W), sc["dtype"], 900 + sc["seed"])])
        _cache[key] = (s, ec.granule(len(s), sc["dtype"]))
    return _cache[key]


def load(eng, dtype, s, ringlen, ftype=1, devptr=None):
    eng.ring_create(ftype, dtype, ringlen, devptr)
    eng.ring_push_raw(ftype, s, len(s))
    assert eng.ring_wrpos(ftype) == len(s)


def trk_states(chans, seed):
    """Open-loop states a few hundred samples into the stream, as tests/test_gpu_lifecycle.py draws them."""
    rng = np.random.default_rng(seed)
    return [dict(carrfreq=c.f_if + float(rng.uniform(-900, 900)), codefreq=c.crate + float(rng.uniform(-2, 2)),
                 remcode=float(rng.uniform(0.01, 0.99)), remcarr=float(rng.uniform(0, 6.2)), buffloc=100 + 900 * i)
            for i, c in enumerate(chans)]


def loop_states(eng, acqfreq=None):
    """Loop states of the engine's channels before bit synchronisation, as tests/test_gpu_loop.py sets them."""
    return [eng.loop_state(i, c.f_if + 200.0 * (i + 1) if acqfreq is None else acqfreq[i], flagsync=0,
                           synci=(3 + 5 * i) % 20, cnt=2001 + 7 * i) for i, c in enumerate(eng.channels)]


def start_states(eng):
    """The tracking states that go with loop_states(): sdracquisition()'s hand-over at the loop's acqfreq."""
    return [dict(carrfreq=c.f_if + 200.0 * (i + 1), codefreq=c.crate, remcode=0.0, remcarr=0.0, buffloc=50 + 700 * i)
            for i, c in enumerate(eng.channels)]


# ---- observations: everything a caller can fetch, in one nested value -------------------------------------------------
def obs_batches(eng, states, lengths):
    """Open-loop batches of the given lengths from `states` (a repeated length runs on the look-ahead plan)."""
    eng.trk_set_state(states)
    out = []
    for n in lengths:
        eng.trk_run(n)
        out.append(eng.trk_fetch() + eng.trk_fetch_sums())
    return dict(batches=out, state=eng.trk_get_state())


def obs_loop(eng, chunks, states=None, loops=None):
    """A closed loop in chunks; states / loops None: from the states the engine holds (after a hand-over)."""
    if states is not None:
        eng.trk_set_state(states)
    if loops is not None:
        eng.loop_set(loops)
    out = []
    for n in chunks:
        eng.trk_run_loop(n)
        out.append(eng.trk_fetch() + eng.trk_fetch_log())
    return dict(chunks=out, state=eng.trk_get_state(), loop=eng.loop_get(), lapped=eng.trk_loop_lapped())


def obs_search(eng, wrpos, power_ch=0, channels=None):
    eng.acq_run(wrpos, channels)
    return dict(res=eng.acq_fetch(), edge=eng.acq_fetch_edge(), fine=eng.acq_fetch_fine(prompts=True),
                power=eng.acq_power(power_ch))


def obs_rx(eng):
    """After a scheduling step: the schedule, the monitor, the tracked periods."""
    lock, losses = eng.rx_lock_status()
    return dict(status=eng.rx_status(), lock=lock, losses=losses, trk=eng.trk_fetch(), log=eng.trk_fetch_log(),
                state=eng.trk_get_state(), loop=eng.loop_get())


def check_margins(w, where=""):
    """The input condition of a search that is held against the oracle: acq_cases.check_margins (every decision MARGIN
    apart) for a search without hypotheses, acq_edge_cases.check_margins (which also bounds tied hypotheses, and asks
    2 * MARGIN of the rows they can move) for one with."""
    (ec.check_margins if w["estep"] > 0 else ac.check_margins)(w, where)


def acquired(res):
    return [int(r["flagacq"]) for r in res]


def check_search(res, chans, want, where=""):
    """The oracle anchor of a search: acq_cases.check_result per channel (decisions exact, peakr and cn0 to 1e-4)."""
    for c, r in zip(chans, res):
        ac.check_result(r, want[c.prn], (where, c.prn))


# ---- oracle anchors of the trackers ----------------------------------------------------------------------------------
def anchor_batches(orc, chans, s, ringlen, states, got, nbatch):
    """The first nbatch batches of obs_batches against orc_sdrtracking, period by period: II, QQ and the sample counts
    bit for bit (the bar of tests/test_gpu_tracking.py)."""
    ring = orc.make_ring(s, ringlen, len(s))
    for i, (c, st) in enumerate(zip(chans, states)):
        o = orc.make_chan(c.prn, dtype=c.dtype, f_sf=c.f_sf, f_if=c.f_if, corrn=c.corrn, corrd=c.corrd, corrp=c.corrd)
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
        b = st["buffloc"]
        for k in range(nbatch):
            II, QQ, ns = got["batches"][k][:3]
            for e in range(II.shape[1]):
                orc.lib().orc_sdrtracking(C.byref(o), C.byref(ring), b)
                assert ns[i, e] == o.currnsamp, (i, k, e)
                assert np.array_equal(II[i, e], np.ctypeslib.as_array(o.II)[:c.ntap]), (i, k, e)
                assert np.array_equal(QQ[i, e], np.ctypeslib.as_array(o.QQ)[:c.ntap]), (i, k, e)
                b += o.currnsamp


FILTER_FIELDS = ("carrfreq", "codefreq", "carrNco", "codeNco", "carrErr", "codeErr", "freqErr")


def anchor_loop(orc, chans, s, ringlen, states, loops, got):
    """obs_loop against the oracle's sdrthread() step, period by period, with the bars of tests/test_gpu_loop.py:
    correlator sums, sample counts, filter flags, NCO remainders and the nav-bit columns bit for bit; the filter
    outputs, which inherit the last bit of the maths library's atan, to 1e-14 from identical inputs, then adopted."""
    ring = orc.make_ring(s, ringlen, len(s))
    for i, (c, st, lp) in enumerate(zip(chans, states, loops)):
        o = orc.make_chan(c.prn, dtype=c.dtype, f_sf=c.f_sf, f_if=c.f_if, corrn=c.corrn, corrd=c.corrd, corrp=c.corrd)
        o.acq.acqfreq = lp.acqfreq
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
        o.flagsync, o.synci, o.cnt = lp.flagsync, lp.synci, lp.cnt
        b = C.c_uint64(st["buffloc"])
        for k, (II, QQ, ns, log, ndone) in enumerate(got["chunks"]):
            assert ndone[i] == II.shape[1], (i, k, ndone)
            for e in range(II.shape[1]):
                where = (i, k, e)
                assert orc.lib().orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(b)) == 1, where
                assert ns[i, e] == o.currnsamp, where
                assert np.array_equal(II[i, e], np.ctypeslib.as_array(o.II)[:c.ntap]), where
                assert np.array_equal(QQ[i, e], np.ctypeslib.as_array(o.QQ)[:c.ntap]), where
                r = log[i, e]
                assert r["flagloopfilter"] == o.flagloopfilter and r["flagsync"] == o.flagsync, where
                assert r["remcode"] == o.remcode and r["remcarr"] == o.remcarr, where
                assert r["navbit"] == (o.bit if (o.flagsync and o.swsync) else 0), where
                for f in FILTER_FIELDS:
                    x, y = float(r[f]), getattr(o, f)
                    assert abs(x - y) <= 1e-14 * max(1.0, abs(x), abs(y)), (where, f, x, y)
                    setattr(o, f, x)
        fin = got["state"][i]
        assert fin["buffloc"] == b.value and fin["remcode"] == o.remcode and fin["remcarr"] == o.remcarr, i
        assert got["loop"][i].cnt == o.cnt, i


# ---- the receiver schedule's scenario --------------------------------------------------------------------------------
# The hand-over signal of tests/acq_fine_cases.py (PRN 3 and 14 present, PRN 5 absent; 216 periods of 4092 samples) in a
# ring of 100 periods.  Steps of 20 periods; a failed search is retried 5 ms of samples later; the lock monitor declares
# a channel lost whose nav bit is not synchronised 15 periods after its hand-over (rule 1 of DESIGN.md 3.2b; the other
# rule needs synchronised bits, which 60 periods do not give), so that a channel acquired in one step is lost in the
# next and searched again in the one after: every edge of the schedule is walked within three steps.
RX_RING = 100 * N4
RX_A, RX_B = [3, 14, 5], [14, 5, 3]         # channel order of the configuration before / after
RX_STEP, RX_RETRY_MS = 20, 5
RX_PRM = dict(sync_periods=15, kbits=1, nbad=1, mu_min=2.0)
RX_A_WRPOS = [16 * N4, 37 * N4]             # the live engine's steps before it is reconfigured
# write positions of the compared steps, every search ends at one: 20 periods apart, and from period 37 because the
# restated searches that end there are all decided with MARGIN (the absent PRN's noise rows tie at 36, 38 and 39)
RX_WRPOS = [37 * N4, 57 * N4, 77 * N4, 97 * N4]


def rx_signal(gc, synth):
    return fc.handover_signal(gc, synth)


def rx_chans(gc, prns, corrn):
    return iq4_set(gc, prns, corrn)


def rx_wants(gc, orc, synth):
    """wrpos -> prn -> restated search of the hand-over signal's channels ending at that write position of RX_RING."""
    if "rx" not in _cache:
        sig = rx_signal(gc, synth)
        sc = fc.SCEN["iq4"]
        out = {}
        for wp in RX_WRPOS:
            pairs = [ec.pair(gc, orc, sc, (p,) + G4) for p in RX_A]
            out[wp] = dict(zip(RX_A, ec.restate(orc, pairs, ac.ring_order(sig, RX_RING, wp), RX_RING, wp)))
        _cache["rx"] = out
    return _cache["rx"]


def rx_begin(eng, monitor=True):
    """loop_set, rx_start and the monitor for the engine's channels."""
    eng.loop_set([eng.loop_state(i, 0.0) for i in range(len(eng.channels))])
    eng.rx_start(RX_RETRY_MS)
    if monitor:
        eng.rx_lock_set(RX_PRM)


def rx_feed(eng, sig, wrpos):
    """Push the signal up to write position wrpos."""
    at = eng.ring_wrpos(1)
    assert at <= wrpos
    if wrpos > at:
        eng.ring_push_raw(1, sig[at:wrpos], wrpos - at)


def rx_steps(eng, sig, wrpos_list):
    """One scheduling step at each write position, everything fetched after each."""
    out = []
    for wp in wrpos_list:
        rx_feed(eng, sig, wp)
        eng.rx_step(RX_STEP)
        out.append(obs_rx(eng))
    return out


class DevMem:
    """Caller-owned device memory through the HIP runtime the library is linked against."""

    def __init__(self, gc, nbytes):
        self.hip, self.p = gc.lib(), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(nbytes)) == 0
        assert self.hip.hipMemset(self.p, 0, C.c_size_t(nbytes)) == 0

    def free(self):
        assert self.hip.hipDeviceSynchronize() == 0 and self.hip.hipFree(self.p) == 0
