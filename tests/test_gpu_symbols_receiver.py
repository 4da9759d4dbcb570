"""The reference-named symbols of libgnsscorr.so (include/sdr_compat.h) as a linked receiver drives them: two front
ends and several tap sets behind one combining queue, a refused request beside good ones, channel structs that are
re-initialised at the same address, more structs than the code table keeps, and the 327 680 000-sample ring's wrap --
once more beyond 2^32 samples.  Every result is compared with the oracle's literal loops: sample counts, II / QQ of
every tap, both remainders, the filter outputs, acquisition integers and buffloc exactly; peakr, cn0 and power to 1e-4.
The scenarios are tests/symbol_cases.py; tests/test_symbol_cases.py shows their margins on the oracle.

The order of the tests in this file is load-bearing: they share one receiver (the fixture `rx`), whose files are read
block by block.  The tests at low positions come first (they assert that), the wrap test then advances the rings to
their end, and the two re-initialised-acquisition tests at the bottom replace the default context's ring 1, after
which `rx` no longer describes it.  A new test at low positions goes before test_ring_wrap_of_the_symbol_path."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import symbol_cases as sc
from conftest import rel_err

pytestmark = pytest.mark.gpu
_libc = C.CDLL(None)
_libc.fclose.argtypes = [C.c_void_p]
_libc.fseek.argtypes = [C.c_void_p, C.c_long, C.c_int]


def _close_files(ini):
    for name in ("fp1", "fp2"):
        if getattr(ini, name):
            _libc.fclose(getattr(ini, name))
            setattr(ini, name, None)


def _receiver(gc, files, cfgs, nblocks):
    """rcvinit_file() on one or two files (the [FEND] fields of each from cfgs), nblocks pushed."""
    L = gc.lib()
    ini = sc.set_ini(gc)
    _close_files(ini)
    ini.fend, ini.useif1, ini.useif2 = gc.FEND_FILE, 1, int(len(files) > 1)
    ini.file1 = str(files[0]).encode()
    ini.file2 = str(files[1]).encode() if len(files) > 1 else b""
    for i, cfg in enumerate(cfgs):
        ini.dtype[i], ini.f_sf[i], ini.f_if[i], ini.f_cf[i] = cfg["dtype"], sc.F_SF, cfg["f_if"], sc.F_CF
    assert L.rcvinit_file(C.byref(ini)) == 0
    for _ in range(nblocks):
        L.file_pushtomembuf()
    st = gc.sdrstat()
    assert st.buffcnt == nblocks and st.fendbuffsize == sc.BLK
    return ini


@pytest.fixture(scope="module")
def rec(gc, synth):
    os.environ["GNSSCORR_ACQSLEEP_MS"] = "0"
    return sc.recordings(gc, synth)


@pytest.fixture(scope="module")
def rx(gc, orc, rec, tmp_path_factory):
    """RX2 with the low blocks pushed; .rings: the oracle's view of the two rings (no wrap yet: the files as they are)."""
    d = tmp_path_factory.mktemp("rx2")
    files = [d / "if1.dat", d / "if2.dat"]
    for f, r in zip(files, rec):
        r.tofile(f)
    ini = _receiver(gc, files, (sc.IF1, sc.IF2), sc.NB_LOW)

    class Rx:
        pass
    r = Rx()
    r.ini, r.rec = ini, rec
    r.rings = [orc.make_ring(b, sc.RINGLEN, sc.NB_LOW * sc.BLK) for b in rec]
    yield r
    _close_files(ini)
    ini.useif2 = 0


def _low_positions(gc):
    assert gc.sdrstat().buffcnt == sc.NB_LOW, "runs before the ring is advanced to its end (file order)"


def _start(gc, orc, c, fpos0, salt=0, sdr=None, chno=1, dfreq=0.0, shift=0):
    """A struct and an oracle channel for c, handed over at the same state; shift: absolute position - file position."""
    sdr = sc.init_sdr(gc, c, sdr=sdr, chno=chno)
    o = sc.oracle_chan(orc, c)
    acqfreq, b = sc.start_state(c, fpos0, salt)
    sc.hand_over(sdr, acqfreq + dfreq, sdr.crate)
    sc.hand_over(o, acqfreq + dfreq, o.crate)
    assert (sdr.clen, sdr.nsamp, sdr.crate, sdr.trk.corrn) == (o.clen, o.nsamp, o.crate, o.corrn)
    return sdr, o, b + shift


def _run_threads(jobs):
    """One thread per job, released together; re-raises the first failure."""
    errs, bar = [], threading.Barrier(len(jobs))

    def run(i):
        try:
            bar.wait()
            jobs[i]()
        except Exception as e:          # noqa: BLE001
            errs.append((i, repr(e)))
    ts = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


def _combined(gc, before, nreq, what):
    """The combiner's counters since `before`: every request served, and at least one chain served several."""
    after = gc.cmb_stats()
    chains, reqs = after[0] - before[0], after[1] - before[1]
    print(f"\n{what}: {reqs} requests in {chains} launch chains ({reqs / max(chains, 1):.2f} each)")
    assert reqs == nreq, (reqs, nreq)
    assert chains < reqs, f"{what}: the threads were served one by one ({chains} chains for {reqs} requests): combining was not exercised"


def test_two_front_ends_several_groups_one_queue(gc, orc, rx):
    """Case 1: 17 channel threads on two rings, L1 C/A and GLONASS G1, tap sets A, B (same corrn, other spacing) and C
    (other corrn): a combined batch splits into up to four groups."""
    _low_positions(gc)
    L = gc.lib()
    chans = sc.MIXED
    trio = [_start(gc, orc, c, 0, chno=i + 1) for i, c in enumerate(chans)]
    got = [None] * len(chans)

    def job(i):
        def f():
            got[i] = sc.symbol_track(gc, trio[i][0], trio[i][2], sc.MIXED_NPER)[0]
        return f
    L.sdrtracking(C.byref(gc.SdrCh()), 1 << 60, 0)          # (context creation outside the threads)
    before = gc.cmb_stats()
    _run_threads([job(i) for i in range(len(chans))])
    _combined(gc, before, len(chans) * sc.MIXED_NPER, "mixed receiver")
    for c, (sdr, o, b), rows in zip(chans, trio, got):
        want, _ = sc.oracle_track(orc, o, rx.rings[c["ring"] - 1], b, sc.MIXED_NPER)
        for k, (g, w) in enumerate(zip(rows, want)):
            assert g == w, (c["key"], k, g, w)
        if sc.sat_of(c) is not None:
            assert min(sc.prompt_power(rows)) > sc.POWER_FLOOR
        L.freesdrch(C.byref(sdr))


def test_group_member_keeps_its_own_smax(gc, orc, rx):
    """Case 1's point about corrp, made sharp: eight channels of smax 6 and eight of smax 16 in one (dtype, corrn)
    group, every period started from a state at which a replica walk begun at coff - 16 ci instead of coff - 6 ci puts
    the period's first sample on the other side of a chip edge.  A member given its group's smax_max differs from the
    oracle there."""
    _low_positions(gc)
    L, O = gc.lib(), orc.lib()
    chans = sc.EDGE
    trio = [_start(gc, orc, c, 0, salt=7, chno=i + 1) for i, c in enumerate(chans)]
    got = [None] * len(chans)

    def job(i):
        sdr, _, b = trio[i]

        def f():
            got[i] = sc.edge_track(lambda loc: L.sdrtracking(C.byref(sdr), loc, 0), sdr, b, i)
        return f
    before = gc.cmb_stats()
    _run_threads([job(i) for i in range(len(chans))])
    _combined(gc, before, len(chans) * len(sc.EDGE_STATES), "edge states, smax 6 beside smax 16")
    for i, (c, (sdr, o, b)) in enumerate(zip(chans, trio)):
        want = sc.edge_track(lambda loc: O.orc_sdrtracking(C.byref(o), C.byref(rx.rings[0]), loc), o, b, i)
        for k, (g, w) in enumerate(zip(got[i], want)):
            assert g == w, (c["key"], k, sc.EDGE_STATES[(i + k) % len(sc.EDGE_STATES)], g, w)
        L.freesdrch(C.byref(sdr))


def test_refused_request_beside_good_ones(gc, orc, rx):
    """Case 2: two structs whose dtype is not their ring's are refused by the host-side check on every call -- flagtrk
    0, the correlator outputs, remainders and frequencies untouched -- and the other channels of the same batches stay
    bit-exact."""
    _low_positions(gc)
    L = gc.lib()
    good = sc.REFUSED_GOOD
    trio = [_start(gc, orc, c, 3 * sc.NSAMP, salt=2, chno=i + 1) for i, c in enumerate(good)]
    bad = []
    for c, dtype in ((sc.chan("bad1", 1, "A", 2), 2), (sc.chan("bad2", 2, "A", 10), 1)):
        sdr, _, b = _start(gc, orc, c, 3 * sc.NSAMP, salt=2)
        sdr.dtype = dtype
        sdr.trk.remcode, sdr.trk.remcarr = 0.25, 0.5
        for t in range(5):
            sdr.trk.II[t], sdr.trk.QQ[t] = t + 0.5, -t - 0.25
        bad.append((sdr, b))
    got = [None] * len(good)

    def good_job(i):
        def f():
            got[i] = sc.symbol_track(gc, trio[i][0], trio[i][2], sc.REFUSED_NPER)[0]
        return f

    def bad_job(sdr, b):
        def f():
            keep = (sc.row_of(sdr)[1:], sdr.trk.carrfreq, sdr.trk.codefreq)
            for k in range(sc.REFUSED_NPER):
                sdr.flagtrk = 1
                L.sdrtracking(C.byref(sdr), b + k * sc.NSAMP, k)
                assert sdr.flagtrk == 0
                assert (sc.row_of(sdr)[1:], sdr.trk.carrfreq, sdr.trk.codefreq) == keep
        return f
    before = gc.cmb_stats()
    _run_threads([good_job(i) for i in range(len(good))] + [bad_job(s, b) for s, b in bad])
    _combined(gc, before, len(good) * sc.REFUSED_NPER, "good requests beside refused ones")
    for c, (sdr, o, b), rows in zip(good, trio, got):
        want, _ = sc.oracle_track(orc, o, rx.rings[c["ring"] - 1], b, sc.REFUSED_NPER)
        assert rows == want, c["key"]
        L.freesdrch(C.byref(sdr))
    for sdr, _ in bad:
        L.freesdrch(C.byref(sdr))


def test_struct_reinitialised_while_tracking(gc, orc, rx):
    """Case 3(a): one struct is PRN A, then (freesdrch + initsdrch) PRN B of the same length, then has its code
    overwritten in place by PRN C's (only the combiner's code hash can notice), then becomes a 511-chip GLONASS
    channel on the other ring."""
    _low_positions(gc)
    L = gc.lib()
    ca, cb, cc, cg = sc.REINIT
    n = sc.REINIT_NPER
    sdr, o, b = _start(gc, orc, ca, 0)
    addr = C.addressof(sdr)
    rows, _ = sc.symbol_track(gc, sdr, b, n)
    assert rows == sc.oracle_track(orc, o, rx.rings[0], b, n)[0]
    L.freesdrch(C.byref(sdr))
    sdr, o, b = _start(gc, orc, cb, 0, sdr=sdr)
    assert C.addressof(sdr) == addr
    rows, b = sc.symbol_track(gc, sdr, b, n)
    want, bo = sc.oracle_track(orc, o, rx.rings[0], b - sum(r[0][0] for r in rows), n)
    assert rows == want and b == bo
    chips = np.ascontiguousarray(gc.gencode(cc["prn"], cc["ctype"])[0], np.int16)
    C.memmove(sdr.code, chips.ctypes.data, chips.nbytes)
    for i, v in enumerate(chips):
        o.code[i] = int(v)
    rows, _ = sc.symbol_track(gc, sdr, b, n, cnt0=n)
    want, _ = sc.oracle_track(orc, o, rx.rings[0], b, n)
    assert rows == want
    L.freesdrch(C.byref(sdr))
    sdr, o, b = _start(gc, orc, cg, 0, sdr=sdr)
    assert C.addressof(sdr) == addr and sdr.clen == 511 and sdr.ftype == 2
    rows, _ = sc.symbol_track(gc, sdr, b, n)
    assert rows == sc.oracle_track(orc, o, rx.rings[1], b, n)[0]
    assert min(sc.prompt_power(rows)) > sc.POWER_FLOOR
    L.freesdrch(C.byref(sdr))


def test_more_structs_than_the_code_table_keeps(gc, orc, rx):
    """Case 5: 250 structs tracked a period each, then two threaded batches that mix known and new structs (264 in all) and
    take the table past its 256 entries; every period of every struct equals the oracle's."""
    _low_positions(gc)
    L = gc.lib()
    trio, rows = {}, {}

    def add(i):
        trio[i] = _start(gc, orc, sc.many_chan(i), 0, salt=i, chno=i + 1, dfreq=200.0 * (i % 5 - 2))
        rows[i] = []

    def step(i, nper):
        sdr, _, b = trio[i]
        b += sum(r[0][0] for r in rows[i])
        rows[i] += sc.symbol_track(gc, sdr, b, nper, cnt0=len(rows[i]))[0]
    for i in range(sc.MANY_FIRST):
        add(i)
        step(i, 1)
    nxt = sc.MANY_FIRST
    for batch, nknown in enumerate(sc.MANY_KNOWN):
        known = list(range(20 * batch, 20 * batch + nknown))
        new = list(range(nxt, nxt + sc.MANY_BATCH - nknown))
        nxt += len(new)
        for i in new:
            add(i)
        before = gc.cmb_stats()
        _run_threads([(lambda i=i: step(i, 2)) for i in known + new])
        _combined(gc, before, 2 * sc.MANY_BATCH, f"batch {batch} of known and new structs")
    assert len(trio) > 256
    for i, (sdr, o, b) in trio.items():
        want, _ = sc.oracle_track(orc, o, rx.rings[0], b, len(rows[i]))
        assert rows[i] == want, i
        L.freesdrch(C.byref(sdr))


@pytest.mark.parametrize("lap", sc.WRAP_LAPS)
def test_ring_wrap_of_the_symbol_path(gc, orc, rx, lap):
    """Case 4: ring and sdrstat.buffcnt advanced together to four blocks short of a multiple of MEMBUFFLEN *
    FILE_BUFFSIZE, six more blocks pushed: searches whose look-back window straddles the ring's end, periods that
    start before it and finish after it, rcvgetbuff() across it, and the host ring against the HBM ring.  lap 14: the
    same where fendbuffsize * buffcnt no longer fits 32 bits."""
    L, O = gc.lib(), orc.lib()
    fb0, cnt0 = sc.wrap_segment(lap)
    st, ctx = gc.sdrstat(), L.gnsscorr_default_ctx()
    jump = cnt0 - st.buffcnt
    assert jump > 0, "laps run in ascending order"
    for ftype, fp, dtype in ((1, rx.ini.fp1, 1), (2, rx.ini.fp2, 2)):
        assert _libc.fseek(fp, fb0 * sc.BLK * dtype, 0) == 0
        assert L.gnsscorr_ring_commit(ctx, ftype, jump * sc.BLK) == 0
    st.buffcnt = cnt0
    for _ in range(sc.NB_WRAP):
        L.file_pushtomembuf()
    wrpos = (cnt0 + sc.NB_WRAP) * sc.BLK
    assert st.buffcnt * st.fendbuffsize == wrpos and L.gnsscorr_ring_wrpos(ctx, 1) == wrpos == L.gnsscorr_ring_wrpos(ctx, 2)
    end = lap * sc.RINGLEN
    assert (wrpos > 1 << 32) == (lap == 14)
    shift = cnt0 * sc.BLK - fb0 * sc.BLK                        # absolute position - file position
    # the oracle's rings: the six blocks where the receiver put them
    rings = []
    for r in rx.rec:
        big = np.zeros((sc.RINGLEN,) + r.shape[1:], np.int8)
        for j in range(sc.NB_WRAP):
            at = (cnt0 + j) % sc.MEMBUFFLEN * sc.BLK
            big[at:at + sc.BLK] = r[(fb0 + j) * sc.BLK:(fb0 + j + 1) * sc.BLK]
        rings.append((big, orc.make_ring(big, sc.RINGLEN, wrpos)))
    # searches on ring 1
    for p in sc.WRAP_ACQ:
        c = sc.chan("w", 1, "A", p)
        sdr = sc.init_sdr(gc, c)
        power = np.zeros(sdr.acq.nfreq * sdr.nsamp)
        buffloc = L.sdracquisition(C.byref(sdr), power.ctypes.data)
        want = sc.oracle_acq_full(orc, sc.oracle_chan(orc, c), rings[0][1])
        print(f"\nlap {lap} PRN {p}: flagacq {sdr.flagacq} codei {sdr.acq.acqcodei} freqi {sdr.acq.freqi} peakr {sdr.acq.peakr:.4f} "
              f"(oracle {want['peakr']:.4f}, iteration {want['iters']}), power rel err {rel_err(power, want['power']):.3g}")
        sc.check_acq(sdr, buffloc, want, (lap, p))
        assert rel_err(power, want["power"]) < 1e-4
        L.freesdrch(C.byref(sdr))
    # periods across the end, both rings
    for i, c in enumerate(sc.WRAP_TRK):
        sdr, o, b = _start(gc, orc, c, end - shift - sc.WRAP_TRK_BACK, salt=lap, chno=i + 1, shift=shift)
        assert b < end
        rows, b1 = sc.symbol_track(gc, sdr, b, sc.WRAP_NPER)
        assert b1 > end
        want, _ = sc.oracle_track(orc, o, rings[c["ring"] - 1][1], b, sc.WRAP_NPER)
        for k, (g, w) in enumerate(zip(rows, want)):
            assert g == w, (lap, c["key"], k)
        if sc.sat_of(c) is not None:
            assert min(sc.prompt_power(rows)) > sc.POWER_FLOOR
        L.freesdrch(C.byref(sdr))
    # rcvgetbuff() across the end; the host ring and the HBM ring hold the same bytes
    n = 5000
    for ftype, dtype in ((1, 1), (2, 2)):
        for loc in (end - 1000, end - n, end, wrpos - n):
            a, b, d = (np.full(n * dtype, 99, np.int8) for _ in range(3))
            assert L.rcvgetbuff(C.byref(rx.ini), loc, n, ftype, dtype, a.ctypes.data) == 0
            O.orc_getbuff(C.byref(rings[ftype - 1][1]), loc, n, dtype, b.ctypes.data)
            assert L.gnsscorr_ring_read(ctx, ftype, loc, n, d.ctypes.data) == 0
            assert np.array_equal(a, b) and np.array_equal(a, d), (lap, ftype, loc)


def _one_ring(gc, rec_i, cfg, path):
    rec_i[:sc.ACQ_NBLOCKS * sc.BLK].tofile(path)
    return _receiver(gc, [path], (cfg,), sc.ACQ_NBLOCKS)


def _search(gc, orc, sdr, c, buf):
    """sdracquisition() on the struct against the oracle's search for channel c on the same samples."""
    want = sc.oracle_acq_full(orc, sc.oracle_chan(orc, c), orc.make_ring(buf, sc.RINGLEN, sc.ACQ_NBLOCKS * sc.BLK))
    assert want["flagacq"] == 1
    buffloc = gc.lib().sdracquisition(C.byref(sdr), None)
    print(f"\nPRN {c['prn']}: sdracquisition() codei {sdr.acq.acqcodei} freqi {sdr.acq.freqi} acqfreq {sdr.acq.acqfreq:.1f} "
          f"peakr {sdr.acq.peakr:.3f} buffloc {buffloc}; oracle codei {want['acqcodei']} freqi {want['freqi']} "
          f"acqfreq {want['acqfreq']:.1f} peakr {want['peakr']:.3f} buffloc {want['buffloc']}")
    sc.check_acq(sdr, buffloc, want, c["prn"])
    assert sdr.trk.carrfreq == want["acqfreq"] and sdr.trk.codefreq == sdr.crate


def test_reinitialised_struct_is_searched_as_the_new_channel(gc, orc, rec, tmp_path):
    """Case 3(b), one ring: sdracquisition() as PRN A; freesdrch() + initsdrch() as PRN B at the same address and
    sdracquisition() again gives the oracle's PRN B; then initsdrch() as PRN A once more with no freesdrch() of the
    library in between (a receiver that links its own), which only the engine's remembered identity can notice."""
    L = gc.lib()
    ini = _one_ring(gc, rec[0], sc.IF1, tmp_path / "if1.dat")
    ca, cb = sc.chan("acq", 1, "A", sc.ACQ_A), sc.chan("acq", 1, "A", sc.ACQ_B)
    sdr = sc.init_sdr(gc, ca)
    addr = C.addressof(sdr)
    _search(gc, orc, sdr, ca, rec[0])
    L.freesdrch(C.byref(sdr))
    sc.init_sdr(gc, cb, sdr=sdr)
    assert C.addressof(sdr) == addr and sdr.flagacq == 0
    _search(gc, orc, sdr, cb, rec[0])
    old = gc.SdrCh.from_buffer_copy(sdr)            # (the allocations of the struct as PRN B)
    C.memset(C.byref(sdr), 0, C.sizeof(sdr))
    sc.init_sdr(gc, ca, sdr=sdr)
    _search(gc, orc, sdr, ca, rec[0])
    L.freesdrch(C.byref(old))
    L.freesdrch(C.byref(sdr))
    _close_files(ini)


def test_reinitialised_struct_after_a_second_rcvinit(gc, orc, rec, tmp_path):
    """Case 3(c): the rings are re-created by a second rcvinit_file() with another front end (ring 1 now int8 IQ at zero
    IF), the struct is set up again at the same address for it: the search runs on the new ring with the new
    channel's dtype, IF and grid."""
    L = gc.lib()
    ini = _one_ring(gc, rec[0], sc.IF1, tmp_path / "if1.dat")
    ca = sc.chan("acq", 1, "A", sc.ACQ_A)
    sdr = sc.init_sdr(gc, ca)
    _search(gc, orc, sdr, ca, rec[0])
    ini = _one_ring(gc, rec[1], sc.IF2, tmp_path / "if2.dat")          # ring 1 again, other sample type
    old = gc.SdrCh.from_buffer_copy(sdr)
    C.memset(C.byref(sdr), 0, C.sizeof(sdr))
    sc.set_ini(gc, "A")
    assert L.initsdrch(1, sc.SYS_GPS, sc.ACQ_C, sc.CTYPE_L1CA, 2, 1, sc.F_CF, sc.F_SF, 0.0, C.byref(sdr)) == 0
    _search(gc, orc, sdr, sc.chan("acq", 2, "A", sc.ACQ_C), rec[1])    # (the oracle's channel: IQ at zero IF)
    L.freesdrch(C.byref(old))
    # and the same front end once more: same sample type and ring length, the engine of PRN C must not outlive it
    ini = _one_ring(gc, rec[1], sc.IF2, tmp_path / "if2b.dat")
    _search(gc, orc, sdr, sc.chan("acq", 2, "A", sc.ACQ_C), rec[1])
    L.freesdrch(C.byref(sdr))
    _close_files(ini)
