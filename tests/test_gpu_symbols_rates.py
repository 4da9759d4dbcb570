"""sdrtracking() and sdracquisition() of libgnsscorr.so (include/sdr_compat.h) at the sample rates of other front ends and
at long code periods, against the oracle's literal loops.  The scenarios are tests/symbol_rate_cases.py;
tests/test_symbol_rate_cases.py shows on the oracle that each is what it claims.

A. The combining queue (gnsscorr_compat.hip: cmb_reserve, cmb_run_group) at periods of 2048 .. 262144 samples, i.e. at
   1 .. 11 segments: its buffers regrow, a short member beside a long one gets empty segments, the sums come back
   through the mapped buffer indexed by the queue's capacity.  currnsamp, II / QQ of every tap, both remainders and the
   frequencies behind the filters equal the oracle's, with ==.
B. sdracquisition()'s private engine at 2048, 8183, 16384, 16385 and 32768 samples (symbol_cases.check_acq's bars, power
   to 1e-4), six tracked periods behind each hand-over, the refusal above 32768 samples, one struct address across
   rates, an absent PRN.

The module's receiver keeps gnsscorr_debug_poison(0xA5) on for the default context: whatever the queue allocates while
growing starts as 0xA5, not as zeros.  The queue's buffers are process-wide and only ever grow, so the growth itself
happens once per process, at whichever test first asks for more segments -- in this module or in another.  No test
here depends on the state it finds: A.1's sequence forces every growth from any smaller state and is served from a
larger one otherwise.

The order of the tests is load-bearing in one respect: the tests of part A and the refused search share the receiver
`rx` (they assert that they still have it); every test of part B sets up a receiver of its own and comes after them."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

import period_edge_cases as pe
import symbol_cases as sc
import symbol_rate_cases as rc
from conftest import rel_err
from test_gpu_symbols_receiver import _close_files, _combined, _run_threads

pytestmark = pytest.mark.gpu
_step1 = {}                     # A.1's rows by channel key, for A.4


def _receiver(gc, files, nblocks):
    """rcvinit_file() on {ring: (path, dtype)}, nblocks pushed.  The [FEND] sample rate is nominal: no ring reads it."""
    L = gc.lib()
    ini = sc.set_ini(gc)
    _close_files(ini)
    ini.fend, ini.useif1, ini.useif2 = gc.FEND_FILE, int(1 in files), int(2 in files)
    ini.file1 = str(files[1][0]).encode() if 1 in files else b""
    ini.file2 = str(files[2][0]).encode() if 2 in files else b""
    for ring, (_, dtype) in files.items():
        ini.dtype[ring - 1], ini.f_sf[ring - 1], ini.f_if[ring - 1], ini.f_cf[ring - 1] = dtype, sc.F_SF, 0.0, sc.F_CF
    assert L.rcvinit_file(C.byref(ini)) == 0
    for _ in range(nblocks):
        L.file_pushtomembuf()
    st = gc.sdrstat()
    assert st.buffcnt == nblocks and st.fendbuffsize == sc.BLK
    return ini


@pytest.fixture(scope="module")
def rx(gc, tmp_path_factory):
    """Ring 1 real samples, ring 2 int8 IQ, rc.NBLK blocks each; allocations poisoned for the whole module."""
    os.environ["GNSSCORR_ACQSLEEP_MS"] = "0"
    L = gc.lib()
    d = tmp_path_factory.mktemp("rates")
    files = {}
    for ring, buf in zip((1, 2), rc.ring_samples()):
        files[ring] = (d / ("if%d.dat" % ring), ring)
        buf.tofile(files[ring][0])
    ctx = L.gnsscorr_default_ctx()
    assert L.gnsscorr_debug_poison(ctx, 0xA5) == 0
    ini = _receiver(gc, files, rc.NBLK)
    yield ini
    L.gnsscorr_debug_poison(ctx, -1)
    _close_files(ini)
    ini.useif2 = 0


def _tracking_rings(gc):
    assert gc.sdrstat().buffcnt == rc.NBLK, "runs before part B replaces the receiver (file order)"


def _struct(gc, c, salt=0, state=None, chno=1):
    """(struct, buffloc): initsdrch() for c, handed over at its start state."""
    sdr = sc.init_sdr(gc, c, chno=chno)
    assert sdr.nsamp == c["nsamp"] and sdr.nsampchip == c["nsamp"] // sdr.clen
    return sdr, rc.hand_over(sdr, c, salt, state)


def _track(gc, c, nper, salt=0, state=None):
    sdr, b = _struct(gc, c, salt, state)
    rows, _ = sc.symbol_track(gc, sdr, b, nper)
    gc.lib().freesdrch(C.byref(sdr))
    return rows


def _equal(rows, want, where):
    assert len(rows) == len(want)
    for k, (g, w) in enumerate(zip(rows, want)):
        assert g == w, (where, k, g, w)


def _differing(rows, want):
    """The first period that differs from the oracle's, or None."""
    assert len(rows) == len(want)
    return next((k for k, (g, w) in enumerate(zip(rows, want)) if g != w), None)


# ---- A: the queue across period lengths -----------------------------------------------------------------------------
@pytest.mark.parametrize("ring", (1, 2))
def test_queue_across_period_lengths(gc, orc, rx, ring):
    """A.1: one thread, one struct per length: 16368, the first length of three segments, 65536, 262144 (two consecutive
    periods), 2048, 16368 again -- the queue's segment capacity grows to 2, 3 and 11 (unless the process has grown it
    already) and then serves one-segment periods from buffers sized for eleven."""
    _tracking_rings(gc)
    bad = []
    for c in rc.seq(ring):
        nper = rc.periods(c["nsamp"], rc.SEQ_CAP)
        rows = _track(gc, c, nper)
        if _differing(rows, rc.oracle_rows(orc, c, nper)) is not None:
            bad.append(c["key"])
        _step1[c["key"]] = rows
    assert not bad, f"periods that differ from the oracle's (the whole sequence is run first): {bad}"


@pytest.mark.parametrize("which", rc.BOUNDARIES)
@pytest.mark.parametrize("ring", (1, 2))
def test_periods_on_both_sides_of_a_segment_boundary(gc, orc, rx, ring, which):
    """A.2: currnsamp alternates between n - 1 and n for n = first_nsamp(dtype, 2), the first length an engine gives two
    segments, and for n = first_nsamp + 100, the first the queue launches with two (symbol_rate_cases.queue_nseg):
    there consecutive calls of one struct change the chain's segment count."""
    _tracking_rings(gc)
    c, st = rc.boundary(ring, which), rc.BOUNDARY_STATE[ring]
    want = rc.oracle_rows(orc, c, rc.BOUNDARY_NPER, state=st)
    assert {r[0][0] for r in want} == {c["nsamp"] - 1, c["nsamp"]}
    _equal(_track(gc, c, rc.BOUNDARY_NPER, state=st), want, c["key"])


def _pair_in_one_chain(gc, orc, ring):
    """A 2048-sample and a 262144-sample request in one launch chain.  Known by counting, not by timing: a 262144-sample
    request of corrn 6 is released first and keeps the leader busy for the milliseconds its chain takes; the pair
    (corrn 2, smax 6 and 16) is released when it sets out and queues up behind it.  The blocker cannot share a chain
    with the pair (another corrn: another group, and cmb_stats counts a chain per group), so two chains for the three
    requests mean that the pair shared one; three mean that a member arrived late, and the attempt is repeated with
    fresh structs.  Every attempt's results equal the oracle's either way."""
    shared = []
    for k in range(rc.PAIR_TRIES):
        chans = rc.pair(ring, k)
        duo = [_struct(gc, c, salt=k, chno=i + 1) for i, c in enumerate(chans)]
        got, go = [None] * 3, threading.Event()

        def job(i):
            def f():
                if i == 0:
                    go.set()
                else:
                    go.wait()
                got[i] = sc.symbol_track(gc, duo[i][0], duo[i][1], 1)[0]
            return f
        before = gc.cmb_stats()
        _run_threads([job(i) for i in range(3)])
        after = gc.cmb_stats()
        for c, (sdr, _), rows in zip(chans, duo, got):
            _equal(rows, rc.oracle_rows(orc, c, 1, salt=k), (c["key"], "attempt", k))
            gc.lib().freesdrch(C.byref(sdr))
        assert after[1] - before[1] == 3
        shared.append(after[0] - before[0] == 2)
        if shared[-1]:
            break
    print(f"\nring {ring}: 2048 beside 262144 samples in one chain at attempt {len(shared)}")
    assert any(shared), f"ring {ring}: the pair never shared a chain in {rc.PAIR_TRIES} attempts"


def test_short_beside_long_in_one_group(gc, orc, rx):
    """A.3: 24 channel threads on both rings; on each ring one (dtype, corrn 2) group of 2048, 16368, first_nsamp(3) and
    262144 samples under tap sets of smax 6 and 16, and a corrn 6 group of 16368 and 65536: every chain is launched with
    its group's longest period, so the short members' units get empty segments.  The long members finish after two
    periods; the short ones track on in chains of one segment while the queue's segment capacity stays 11."""
    _tracking_rings(gc)
    L = gc.lib()
    chans = rc.mixed(1) + rc.mixed(2)
    duo = [_struct(gc, c, chno=i + 1) for i, c in enumerate(chans)]
    got = [None] * len(chans)

    def job(i):
        def f():
            got[i] = sc.symbol_track(gc, duo[i][0], duo[i][1], rc.mixed_nper(chans[i]))[0]
        return f
    L.sdrtracking(C.byref(gc.SdrCh()), 1 << 60, 0)          # (context creation outside the threads)
    before = gc.cmb_stats()
    _run_threads([job(i) for i in range(len(chans))])
    _combined(gc, before, sum(rc.mixed_nper(c) for c in chans), "2048 .. 262144 samples on two rings")
    bad = []
    for c, (sdr, _), rows in zip(chans, duo, got):
        k = _differing(rows, rc.oracle_rows(orc, c, rc.mixed_nper(c)))
        if k is not None:
            bad.append((c["key"], k))
        L.freesdrch(C.byref(sdr))
    assert not bad, f"(member, first period that differs from the oracle's): {bad}"
    for ring in (1, 2):
        _pair_in_one_chain(gc, orc, ring)


@pytest.mark.parametrize("ring", (1, 2))
def test_lengths_after_the_mixed_batches(gc, orc, rx, ring):
    """A.4: one thread again, 262144 samples and then 2048: the oracle's rows, and A.1's rows of the same struct state
    (when A.1 ran in this process)."""
    _tracking_rings(gc)
    for c in rc.after(ring):
        nper = rc.periods(c["nsamp"], rc.SEQ_CAP)
        rows = _track(gc, c, nper)
        _equal(rows, rc.oracle_rows(orc, c, nper), c["key"])
        if c["key"] in _step1:
            assert rows == _step1[c["key"]], c["key"]


# ---- B: sdracquisition() at the transform lengths -------------------------------------------------------------------
def _printed(capfd):
    """What the library's printf has written since the last call (its stdio buffer flushed first)."""
    C.CDLL(None).fflush(None)
    return capfd.readouterr().out


def test_search_refused_above_32768_samples_tracking_is_not(gc, orc, rx, capfd):
    """A 65.536 Msps struct: sdracquisition() prints one error line and returns wrpos - (intg + 1) * nsamp with flagacq,
    acq.* and trk.carrfreq as they were and without ACQSLEEP's pause (set to 5 s here: a refusal that slept would take
    that long); after a manual hand-over sdrtracking() tracks the same struct bit for bit."""
    _tracking_rings(gc)
    L = gc.lib()
    c = rc.rate_chan("refused", 2, "A", 21, rc.REFUSED_NSAMP)
    sdr = sc.init_sdr(gc, c)
    assert sdr.nsamp == rc.REFUSED_NSAMP and sdr.acq.intg == rc.ACQ_INTG
    sdr.acq.acqcodei, sdr.acq.freqi, sdr.acq.acqfreq, sdr.acq.cn0, sdr.acq.peakr = 77, 5, 1234.5, 33.25, 1.75
    sdr.trk.carrfreq = 4321.5
    keep = lambda: (sdr.flagacq, sdr.acq.acqcodei, sdr.acq.freqi, sdr.acq.acqfreq, sdr.acq.cn0, sdr.acq.peakr,   # noqa: E731
                    sdr.trk.carrfreq, sdr.trk.codefreq)
    was = keep()
    _printed(capfd)
    os.environ["GNSSCORR_ACQSLEEP_MS"] = "5000"
    try:
        t0 = time.perf_counter()
        buffloc = L.sdracquisition(C.byref(sdr), None)
        dt = time.perf_counter() - t0
    finally:
        os.environ["GNSSCORR_ACQSLEEP_MS"] = "0"
    out = _printed(capfd)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("error: sdracquisition:"), out
    assert buffloc == rc.WRPOS - (rc.ACQ_INTG + 1) * rc.REFUSED_NSAMP
    assert keep() == was and sdr.flagacq == 0
    assert dt < 2.5, dt
    o = sc.oracle_chan(orc, c)
    acqfreq, _ = rc.start(c)
    sc.hand_over(sdr, acqfreq, sdr.crate)
    sc.hand_over(o, acqfreq, o.crate)
    rows, _ = sc.symbol_track(gc, sdr, buffloc, rc.REFUSED_NPER)
    want, _ = sc.oracle_track(orc, o, orc.make_ring(rc.ring_samples()[1], sc.RINGLEN, rc.WRPOS), buffloc, rc.REFUSED_NPER)
    _equal(rows, want, "65536 samples")
    L.freesdrch(C.byref(sdr))


def _one_ring(gc, buf, dtype, path):
    """A receiver of one ring (ring 1 for real samples, ring 2 for IQ) that holds the whole recording."""
    buf.tofile(path)
    return _receiver(gc, {dtype: (path, dtype)}, len(buf) // sc.BLK)


def _rate_struct(gc, c, sdr=None):
    sdr = rc.cut_grid(sc.init_sdr(gc, c, sdr=sdr), c)
    assert sdr.nsamp == c["nsamp"] and sdr.acq.nfreq == 5 and sdr.flagacq == 0
    return sdr


def _search(gc, orc, sdr, name, buf, prn=None, power=None):
    """sdracquisition() on the struct against the oracle's search of the rate's channel over the same samples.  Returns
    (oracle channel after its search, its result, buffloc)."""
    o, want = rc.oracle_search(orc, name, buf, prn)
    buffloc = gc.lib().sdracquisition(C.byref(sdr), None if power is None else power.ctypes.data)
    print(f"\n{name} PRN {sdr.prn}: flagacq {sdr.flagacq} codei {sdr.acq.acqcodei} freqi {sdr.acq.freqi} peakr {sdr.acq.peakr:.4f} "
          f"buffloc {buffloc}; oracle flagacq {want['flagacq']} codei {want['acqcodei']} freqi {want['freqi']} "
          f"peakr {want['peakr']:.4f} buffloc {want['buffloc']} (iteration {want['iters']})")
    sc.check_acq(sdr, buffloc, want, name)
    if want["flagacq"]:
        assert sdr.trk.carrfreq == want["acqfreq"] and sdr.trk.codefreq == sdr.crate
    return o, want, buffloc


@pytest.mark.parametrize("name", list(rc.RATES))
def test_search_then_track_at_rate(gc, orc, synth, rx, tmp_path, name):
    """RTL-SDR replay (2048 samples IQ, two per chip), GN3S (8183 real, prime), 16384 (the 32768-point transform
    unpadded), 16385 (forces 65536 points) and 32768 IQ (the longest search): a receiver of its own per rate, the
    search against the oracle's, then sdrthread's loop on the handed-over struct for six periods."""
    L = gc.lib()
    r, buf = rc.RATES[name], rc.acq_recording(gc, synth, name)
    ini = _one_ring(gc, buf, r["dtype"], tmp_path / "if.dat")
    sdr = _rate_struct(gc, rc.acq_chan(name))
    power = np.zeros(sdr.acq.nfreq * sdr.nsamp)
    o, want, buffloc = _search(gc, orc, sdr, name, buf, power=power)
    assert want["flagacq"] == 1 and want["iters"] == 1
    print(f"{name}: power rel err {rel_err(power, want['power']):.3g}")
    assert rel_err(power, want["power"]) < 1e-4
    rows, _ = sc.symbol_track(gc, sdr, buffloc, rc.ACQ_NPER)
    wrows, _ = sc.oracle_track(orc, o, orc.make_ring(buf, sc.RINGLEN, len(buf)), want["buffloc"], rc.ACQ_NPER)
    _equal(rows, wrows, name)
    assert min(sc.prompt_power(rows)) > rc.power_floor(r["nsamp"])
    L.freesdrch(C.byref(sdr))
    _close_files(ini)


def test_absent_prn_at_2048_samples(gc, orc, synth, rx, tmp_path):
    """All ten windows of a PRN that is not there: flagacq 0, the oracle's lag, bin and buffloc."""
    name, prn = rc.ABSENT
    buf = rc.acq_recording(gc, synth, name)
    ini = _one_ring(gc, buf, rc.RATES[name]["dtype"], tmp_path / "if.dat")
    sdr = _rate_struct(gc, rc.acq_chan(name, prn))
    _, want, _ = _search(gc, orc, sdr, name, buf, prn=prn)
    assert want["flagacq"] == 0 and sdr.flagacq == 0 and want["iters"] == rc.ACQ_INTG
    gc.lib().freesdrch(C.byref(sdr))
    _close_files(ini)


def test_one_struct_address_across_rates(gc, orc, synth, rx, tmp_path):
    """sdracquisition() at 16.384 Msps; freesdrch() + initsdrch() at 2.048 Msps at the same address on the re-created
    ring gives the oracle's 2048-sample result; memset + initsdrch() back to 16.384 Msps with no freesdrch() of the
    library in between (a receiver that links its own) on the ring re-created once more; and the same step to 2.048 Msps
    on the ring as it stands -- there the ring's identity cannot have changed, so only the engine's remembered channel
    constants can tell it that the struct is another channel now."""
    L = gc.lib()
    na, nb = rc.REINIT
    bufa, bufb = rc.acq_recording(gc, synth, na), rc.acq_recording(gc, synth, nb)
    dtype = rc.RATES[na]["dtype"]
    ini = _one_ring(gc, bufa, dtype, tmp_path / "a.dat")
    sdr = _rate_struct(gc, rc.acq_chan(na))
    addr = C.addressof(sdr)
    assert _search(gc, orc, sdr, na, bufa)[1]["flagacq"] == 1
    L.freesdrch(C.byref(sdr))
    ini = _one_ring(gc, bufb, dtype, tmp_path / "b.dat")
    _rate_struct(gc, rc.acq_chan(nb), sdr=sdr)
    assert C.addressof(sdr) == addr and sdr.nsamp == rc.RATES[nb]["nsamp"]
    assert _search(gc, orc, sdr, nb, bufb)[1]["flagacq"] == 1
    olds = [gc.SdrCh.from_buffer_copy(sdr)]         # (the allocations of the struct as it was)
    C.memset(C.byref(sdr), 0, C.sizeof(sdr))
    ini = _one_ring(gc, bufa, dtype, tmp_path / "a2.dat")
    _rate_struct(gc, rc.acq_chan(na), sdr=sdr)
    assert _search(gc, orc, sdr, na, bufa)[1]["flagacq"] == 1
    olds.append(gc.SdrCh.from_buffer_copy(sdr))
    C.memset(C.byref(sdr), 0, C.sizeof(sdr))
    _rate_struct(gc, rc.acq_chan(nb), sdr=sdr)
    _search(gc, orc, sdr, nb, bufa)                 # (2048-sample windows of the 16.384 Msps recording: the oracle's, whatever it finds)
    for old in olds:
        L.freesdrch(C.byref(old))
    L.freesdrch(C.byref(sdr))
    _close_files(ini)
