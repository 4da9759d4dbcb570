"""The closed loop (gnsscorr_trk_run_loop) as a receiver runs it, against the oracle (parity tests proper, -m gpu):
one engine that mixes front ends, code types, tap spans and nav-sync states; a ring of a few code periods fed chunk
by chunk while the loop runs; a channel the writer has lapped; and the tap spans on either side of the one at which, at
16.368 Msps, the code step's pieces stop fitting the tail's table (tests/test_gpu_tap_spans.py has every front end).

Bar: the one tests/test_gpu_loop.py sets -- sums, samples per period, remainders, filter-update flags, flagsync and
decided bits bit for bit, filter outputs to 1e-12 with teacher forcing (_adopt), final state equal to the oracle's."""
import ctypes as C

import numpy as np
import pytest

import acq_cases as ac
from test_gpu_loop import _check_against_oracle, _random_states_case

pytestmark = pytest.mark.gpu

F_SF = 16.368e6


def _start(gc, orc, engine, rng, chans, nav):
    """Random start states on noise (as _random_states_case) for `chans`, with nav[i] = (flagsync, synci, cnt).
    Sets the device's tracking and loop states; returns the oracle channels and their bufflocs."""
    states, ochs, bufflocs, loops = [], [], [], []
    for i, c in enumerate(chans):
        edge = i % 4
        remcode = (0.0 if edge == 0 else float(rng.uniform(0.0, 1e-6)) if edge == 1 else
                   float(1.0 - rng.uniform(0.0, 1e-6)) if edge == 2 else float(rng.uniform(0.01, 0.99)))
        st = dict(carrfreq=c.f_if + c.foffset + float(rng.uniform(-9000, 9000)), codefreq=c.crate + float(rng.uniform(-6, 6)),
                  remcode=remcode, remcarr=float(rng.uniform(0, 6.2)) if i % 5 else 0.0, buffloc=int(rng.integers(0, c.nsamp)))
        states.append(st)
        acqfreq = c.f_if + c.foffset + 200.0 * round((st["carrfreq"] - c.f_if - c.foffset) / 200.0)
        o = orc.make_chan(c.prn, ctype=c.ctype, dtype=c.dtype, f_sf=c.f_sf, f_if=c.f_if, corrn=c.corrn,
                          corrd=int(c.corrp[0]), corrp=int(c.corrp[c.ne // 2]) if c.ne else 0)
        assert (o.ne, o.nl, o.loopms, o.rate) == (c.ne, c.nl, engine.loop_state(i, 0.0).loopms, engine.loop_state(i, 0.0).rate)
        o.acq.acqfreq = acqfreq
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
        o.flagsync, o.synci, o.cnt = nav[i]
        ochs.append(o)
        bufflocs.append(C.c_uint64(st["buffloc"]))
        loops.append(engine.loop_state(i, acqfreq, flagsync=nav[i][0], synci=nav[i][1], cnt=nav[i][2]))
    engine.trk_set_state(states)
    engine.loop_set(loops)
    return ochs, bufflocs


def _check_final(engine, ochs, bufflocs, ntap):
    fin = engine.trk_get_state()
    lst = engine.loop_get()
    for i, o in enumerate(ochs):
        assert fin[i]["buffloc"] == bufflocs[i].value and fin[i]["remcode"] == o.remcode and fin[i]["remcarr"] == o.remcarr, i
        for f in ("flagsync", "synci", "navcnt", "swloop", "cnt", "biti", "bit", "swsync", "swreset"):
            assert getattr(lst[i], f) == getattr(o, f), (i, f)
        assert lst[i].bitIP == o.bitIP and list(lst[i].bitsync) == list(o.bitsync), i
        for name in ("sumI", "sumQ", "oldsumI", "oldsumQ", "II", "QQ"):
            assert np.array_equal(np.ctypeslib.as_array(getattr(lst[i], name))[:ntap],
                                  np.ctypeslib.as_array(getattr(o, name))[:ntap]), (i, name)
    return lst


# (ctype name, prn / frequency number, front end, corrd, synced start (synci, cnt)); every channel has corrn = 4, so
# the outermost taps lie at 4, 8, 16 and 28 samples: the tail's code step takes its 8-, 15- and 32-position classes
# side by side.  Front end 1: int8 IQ at 16.368 Msps; front end 2: real samples at 20 Msps on a 4 MHz IF (the longest
# period: max_n and the step's rounds come from it, front end 1's periods use fewer).
MIXED = [
    ("L1CA", 3, 1, 1, None),          # PRN <= 5: checksync's vote branch
    ("L1CA", 17, 1, 2, (4, 2100)),
    ("L1CA", 28, 1, 7, (13, 2207)),
    ("G1", -7, 1, 4, None),           # frequency number <= 5: vote branch
    ("G1", 3, 1, 2, (2, 2013)),
    ("G1", 6, 1, 7, None),            # shift-register branch, rate 10
    ("SBAS", 120, 1, 1, None),        # shift register, rate 2: syncs on noise within a few periods of cnt 2000
    ("SBAS", 133, 1, 4, (1, 2050)),
    ("L1CA", 9, 2, 2, None),
    ("L1CA", 22, 2, 7, (11, 3000)),
    ("G1", -2, 2, 1, (7, 2045)),
    ("SBAS", 138, 2, 4, None),
    ("L1CA", 31, 2, 4, (19, 2400)),
]


@pytest.mark.parametrize("synced", [True, False], ids=["sync_states_mixed", "none_synced_at_start"])
def test_closed_loop_mixed_receiver(gc, orc, engine, synced):
    """13 channels in one engine: two front ends that differ in sample format, rate and IF; L1 C/A, GLONASS G1
    (frequency numbers -7, -2, 3, 6) and SBAS (rate 2, 2-period filter interval); outermost taps at 4, 8, 16 and 28
    samples under one corrn; channels before and after nav bit sync with different synci / cnt phases (filter
    intervals of 1 to 10 periods in one launch) and SBAS channels that synchronise during the run.  Front end 2 gets
    less data than the first run asks for: its channels stop where their data ends while front end 1's run on, and
    resume exactly in the second run after the rest arrives.  97 + 33 periods.
    none_synced_at_start: every channel starts before sync, so the run begins with one period per step and switches
    to intervals of up to 10 periods when the SBAS channels synchronise."""
    nper, chunks, corrn = 130, (97, 33), 4
    ctypes = {"L1CA": gc.CTYPE_L1CA, "G1": gc.CTYPE_G1, "SBAS": gc.CTYPE_L1SBAS}
    fe = {1: dict(dtype=2, f_sf=16.368e6, f_if=0.0), 2: dict(dtype=1, f_sf=20e6, f_if=4e6)}
    rng = np.random.default_rng(4242 + synced)
    data, rings = {}, {}
    for ft, d in fe.items():
        n = int(d["f_sf"] * 1e-3) * (nper + 4)
        data[ft] = rng.integers(-60, 61, size=(n, 2) if d["dtype"] == 2 else (n,), dtype=np.int8)
        engine.ring_create(ft, d["dtype"], n)
    # front end 2: 60 periods and a bit first -- less than the first run needs
    part2 = 20000 * 60 + 777
    engine.ring_push_raw(1, data[1], data[1].shape[0])
    engine.ring_push_raw(2, data[2][:part2], part2)
    rings[1] = orc.make_ring(data[1], data[1].shape[0], data[1].shape[0])
    rings[2] = orc.make_ring(data[2], data[2].shape[0], part2)
    chans, nav = [], []
    for k, (ct, prn, ft, corrd, sync) in enumerate(MIXED):
        chans.append(gc.Channel(prn, ctype=ctypes[ct], ftype=ft, corrn=corrn, corrd=corrd, corrp=corrd * (1 + k % 2), **fe[ft]))
        start = sync if (synced and sync) else None
        nav.append((1, start[0], start[1]) if start else (0, 0, 1994 + 3 * k))
    engine.set_channels(chans)
    assert max(c.nsamp for c in chans) == 20000 and sorted({int(c.corrp[-1]) for c in chans}) == [4, 8, 16, 28]
    ochs, bufflocs = _start(gc, orc, engine, rng, chans, nav)
    oring = [rings[c.ftype] for c in chans]
    ntap = 1 + 2 * corrn
    ndone = _check_against_oracle(orc, engine, ochs, oring, bufflocs, chunks[0], ntap, tol=1e-12, stops=True)
    fe2 = [i for i, c in enumerate(chans) if c.ftype == 2]
    assert all(ndone[i] == chunks[0] for i, c in enumerate(chans) if c.ftype == 1), ndone
    assert all(55 <= ndone[i] <= 61 for i in fe2), ndone
    sbas = [i for i, c in enumerate(chans) if c.ctype == gc.CTYPE_L1SBAS]
    assert all(ochs[i].flagsync == 1 for i in sbas)                    # (the SBAS channels synchronised)
    engine.ring_push_raw(2, data[2][part2:], data[2].shape[0] - part2)
    rings[2].wrpos = data[2].shape[0]
    _check_against_oracle(orc, engine, ochs, oring, bufflocs, chunks[1], ntap, done=chunks[0], tol=1e-12)
    _check_final(engine, ochs, bufflocs, ntap)


def _stream_case(gc, orc, engine, dtype, f_if, seed):
    nsamp = 16368
    R = 3 * nsamp + (1000 if dtype == 2 else 1008)         # a few periods, no multiple of one; dtype*R % 16 == 0
    assert (dtype * R) % 16 == 0 and R % nsamp
    total = 21 * R + 2 * nsamp
    rng = np.random.default_rng(seed)
    full = rng.integers(-60, 61, size=(total, 2) if dtype == 2 else (total,), dtype=np.int8)
    engine.ring_create(1, dtype, R)
    prns = [2, 4, 11, 19, 23, 32]
    chans = [gc.Channel(p, dtype=dtype, f_if=f_if, corrn=2, corrd=3, corrp=3) for p in prns]
    engine.set_channels(chans)
    nav = [(i % 2, (5 * i) % 20, 2001 + 13 * i) for i in range(len(chans))]
    ochs, bufflocs = _start(gc, orc, engine, rng, chans, nav)
    return R, full, ochs, bufflocs, rng


@pytest.mark.parametrize("dtype,f_if", [(2, 0.0), (1, 4.092e6)], ids=["iq", "real_if4M"])
def test_closed_loop_on_a_streamed_ring(gc, orc, engine, dtype, f_if):
    """A ring of three code periods and a bit, fed in chunks of 12000-16800 samples between trk_run_loop calls until
    the write position has gone round it 21 times: periods straddle the ring's end over and over, channels stop where
    the data ends and go on after the next chunk.  Every other chunk is pushed while the previous run's launches are
    still queued (into slots that run does not read: the push must not wait for it, and the run must not see it).
    The oracle reads the whole recording; everything bit for bit."""
    R, full, ochs, bufflocs, rng = _stream_case(gc, orc, engine, dtype, f_if, 77 + dtype)
    ring = orc.make_ring(full, full.shape[0], 0)
    wp, done, k = 0, 0, 0
    ran = np.zeros(len(ochs), np.int64)

    def push(n):
        nonlocal wp
        engine.ring_push_raw(1, full[wp:wp + n], n)
        wp += n

    push(2 * 16368)
    while wp < 21 * R:
        ring.wrpos = wp
        before = min(b.value for b in bufflocs)
        # the next chunk overwrites samples below wp + n - R: not one the run reads (from `before` on)
        n = min(int(rng.integers(12000, 16801)), before + R - wp, full.shape[0] - wp)
        assert n > 0
        queued = k % 2 == 1
        ran += _check_against_oracle(orc, engine, ochs, ring, bufflocs, 3, 5, done=done, stops=True,
                                     between=(lambda: push(n)) if queued else None)
        if not queued:
            push(n)
        # (a period never reads past the write position the run saw: n <= nsamp + 1 here)
        assert all(b.value <= ring.wrpos for b in bufflocs)
        done += 3
        k += 1
    assert wp // R >= 21 and engine.ring_wrpos(1) == wp
    assert k >= 60 and np.all(ran >= (wp - 3 * 16368) // 16368), (k, ran)    # every channel kept up with the writer
    _check_final(engine, ochs, bufflocs, 5)


def test_closed_loop_lapped_channel_is_counted(gc, orc, engine):
    """A channel more than a ring behind the writer reads samples the writer has overwritten since.  trk_run_loop runs
    the period as sdrtracking() runs it on the reference's ring (the oracle on the ring as it holds them, bit for bit)
    and counts it: trk_loop_lapped reports one period (the lapped channel's first; the channel exactly a ring behind
    is not lapped).  The fetches stay clean, so that a caller whose ring repeats one chunk may rewind (bench.py's
    closed-loop leg does), and the next run that reads only held samples counts none."""
    nsamp = 16368
    R = 3 * nsamp + 1000
    rng = np.random.default_rng(31)
    full = rng.integers(-60, 61, size=(2 * R + 5000, 2), dtype=np.int8)
    engine.ring_create(1, 2, R)
    for a, b in ((0, R), (R, 2 * R), (2 * R, 2 * R + 5000)):
        engine.ring_push_raw(1, full[a:b], b - a)
    wp = engine.ring_wrpos(1)
    assert wp == 2 * R + 5000
    held = ac.ring_order(full, R, wp)                           # the ring as the writer left it: sample p at p % R
    ring = orc.make_ring(held, R, wp)
    chans = [gc.Channel(p, dtype=2, f_if=0.0) for p in (5, 14)]
    engine.set_channels(chans)
    b0 = (wp - R - 1, wp - R)
    engine.trk_set_state([dict(carrfreq=1000.0, codefreq=c.crate, remcode=0.25, remcarr=0.5, buffloc=b)
                          for c, b in zip(chans, b0)])
    engine.loop_set([engine.loop_state(i, 1000.0) for i in range(2)])
    ochs = []
    for c in chans:
        o = orc.make_chan(c.prn, dtype=2, f_if=0.0)
        o.acq.acqfreq = o.carrfreq = 1000.0
        o.codefreq, o.remcode, o.remcarr = o.crate, 0.25, 0.5
        o.flagsync, o.synci, o.cnt = 0, 0, 0
        ochs.append(o)
    bufflocs = [C.c_uint64(b) for b in b0]
    _check_against_oracle(orc, engine, ochs, ring, bufflocs, 2, 5)
    assert engine.trk_loop_lapped() == 1
    # the lapped period read other samples than the stream's: the oracle on the whole recording disagrees
    II, _, _ = engine.trk_fetch()
    o = orc.make_chan(5, dtype=2, f_if=0.0)
    o.carrfreq, o.codefreq, o.remcode, o.remcarr = 1000.0, o.crate, 0.25, 0.5
    orc.lib().orc_sdrtracking(C.byref(o), C.byref(orc.make_ring(full, full.shape[0], wp)), b0[0])
    assert not np.array_equal(II[0, 0], np.ctypeslib.as_array(o.II)[:5])
    # both channels are now inside what the ring holds
    _check_against_oracle(orc, engine, ochs, ring, bufflocs, 1, 5, done=2)
    assert engine.trk_loop_lapped() == 0


@pytest.mark.parametrize("flagsync", [0, 1])
def test_closed_loop_outermost_tap_28(gc, orc, engine, flagsync):
    """One tap pair at 28 samples (corrn 1, corrd 28), the widest span whose code table the step itself fills at this
    rate (24 pieces, all the table holds), before and after nav bit sync: 4 channels x 60 periods in two runs against
    the oracle, as test_closed_loop_9_and_33_taps."""
    _random_states_case(gc, orc, engine, 2800 + flagsync, 2, 0.0, F_SF, (1, 28, 28), flagsync, nper=60, nch=4,
                        chunks=(37, 23))


@pytest.mark.parametrize("flagsync", [0, 1])
@pytest.mark.parametrize("span", [29, 30])
def test_closed_loop_outermost_tap_29_and_30_match_the_oracle(gc, orc, engine, span, flagsync):
    """From 29 samples on at this rate the code step's pieces do not fit the tail's table and the walker serves
    (the loop used to report such runs as needing more NCO pieces than the tables hold): the same
    four channels and eight periods, now against the oracle, and the fetch is clean."""
    n = 16368 * 12
    rng = np.random.default_rng(span + flagsync)
    data = rng.integers(-60, 61, size=(n, 2), dtype=np.int8)
    engine.ring_create(1, 2, n)
    engine.ring_push_raw(1, data, n)
    chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=1, corrd=span, corrp=span) for p in (1, 8, 15, 26)]
    engine.set_channels(chans)
    states = [dict(carrfreq=float(rng.uniform(-5000, 5000)), codefreq=c.crate + float(rng.uniform(-3, 3)),
                   remcode=float(rng.uniform(0, 1)), remcarr=float(rng.uniform(0, 6)), buffloc=100 + 999 * i)
              for i, c in enumerate(chans)]
    engine.trk_set_state(states)
    engine.loop_set([engine.loop_state(i, 0.0, flagsync=flagsync, synci=3 * i, cnt=2001) for i in range(4)])
    ochs = []
    for i, (c, st) in enumerate(zip(chans, states)):
        o = orc.make_chan(c.prn, dtype=2, f_if=0.0, corrn=1, corrd=span, corrp=span)
        o.acq.acqfreq = 0.0
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
        o.flagsync, o.synci, o.cnt = flagsync, 3 * i, 2001
        ochs.append(o)
    bufflocs = [C.c_uint64(st["buffloc"]) for st in states]
    _check_against_oracle(orc, engine, ochs, orc.make_ring(data, n, n), bufflocs, 8, 3, tol=1e-12)
    _check_final(engine, ochs, bufflocs, 3)
