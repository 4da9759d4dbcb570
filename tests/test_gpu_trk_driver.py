"""The batched tracker's host driver (gnsscorr_trk.hip, below the kernels): what it keeps per channel set (GcBatch), what
it shares with the closed loop (GcTrkOut, the committed state) and what a new channel set leaves of either.

Every comparison is exact equality between two runs of the same kernels on the same samples: no tolerance anywhere."""
import struct

import numpy as np
import pytest

from test_gpu_lifecycle import NSAMP, _states

pytestmark = pytest.mark.gpu
ESTATE = -3


@pytest.fixture(scope="module")
def noise():
    """int8 IQ noise at 16.368 Msps, 40 code periods: the ring of every engine here."""
    return np.random.default_rng(31).integers(-60, 61, size=(NSAMP * 40, 2), dtype=np.int8)


def _engine(gc, data, chans):
    e = gc.Engine(0)
    e.ring_create(1, 2, data.shape[0])
    e.ring_push_raw(1, data, data.shape[0])
    e.set_channels(chans)
    return e


def _bits(states):
    return [struct.pack("<ddddQ", s["carrfreq"], s["codefreq"], s["remcode"], s["remcarr"], s["buffloc"]) for s in states]


def _loops(eng, states):
    return [eng.loop_state(i, 200.0 * round(s["carrfreq"] / 200.0), flagsync=0, synci=(7 * i) % 20, cnt=2001, loop=1)
            for i, s in enumerate(states)]


def _run(eng, kind, n, loop_from=None):
    """One run and everything it leaves: II, QQ, nsamp, (the log's fields, ndone,) the state afterwards."""
    if kind == "loop":
        eng.loop_set(_loops(eng, loop_from))
        eng.trk_run_loop(n)
    else:
        eng.trk_run(n)
    out = list(eng.trk_fetch())
    if kind == "loop":
        log, ndone = eng.trk_fetch_log()
        out += [log[f] for f in log.dtype.names] + [ndone]
    return out, eng.trk_get_state()


def _same(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def test_batch_loop_batch_on_one_channel_set(gc, noise):
    """3 channels of the 5-tap default: two batches (the second on the look-ahead plan), a closed-loop run that drops
    the plan made ahead, then batches of 4 and 7 (the batch buffers grow), with no trk_set_state in between.  A second
    engine reproduces each run in isolation from the state the first reported just before it."""
    chans = [gc.Channel(p, dtype=2, f_if=0.0) for p in (4, 9, 21)]
    live, ref = _engine(gc, noise, chans), _engine(gc, noise, chans)
    try:
        live.trk_set_state(_states(chans, 41))
        before = live.trk_get_state()
        for step, (kind, n) in enumerate([("batch", 4), ("batch", 4), ("loop", 5), ("batch", 4), ("batch", 7)]):
            a, after = _run(live, kind, n, loop_from=before)
            ref.trk_set_state(before)
            b, after_ref = _run(ref, kind, n, loop_from=before)
            _same(a, b, (step, kind, n))
            assert _bits(after) == _bits(after_ref), (step, kind, n)
            assert _bits(after) != _bits(before), (step, kind, n)           # the run moved the state on
            before = after
    finally:
        live.close()
        ref.close()


def test_loop_on_an_engine_that_never_ran_a_batch_then_a_batch_that_grows(gc, noise):
    """2 channels of 7 taps.  The first engine's first run is a closed-loop one (it has the outputs and no batch buffers
    yet), then batches of 3, 9 (the batch buffers grow while what was planned ahead at length 3 is dropped) and 9.  The
    second engine has every buffer at its final size from a warm-up batch of 9 from a throw-away state."""
    chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=3, corrd=3, corrp=3) for p in (6, 17)]
    start = _states(chans, 43)
    cold, warm = _engine(gc, noise, chans), _engine(gc, noise, chans)
    try:
        warm.trk_set_state(_states(chans, 44))
        warm.trk_run(9)
        warm.trk_fetch()
        for e in (cold, warm):
            e.trk_set_state(start)
        for step, (kind, n) in enumerate([("loop", 6), ("batch", 3), ("batch", 9), ("batch", 9)]):
            a, sa = _run(cold, kind, n, loop_from=start)
            b, sb = _run(warm, kind, n, loop_from=start)
            _same(a, b, (step, kind, n))
            assert _bits(sa) == _bits(sb), (step, kind, n)
    finally:
        cold.close()
        warm.close()


def test_fetch_after_reconfiguration(gc, noise):
    """After set_channels on a used engine there is no completed run to fetch: GNSSCORR_ESTATE, as on a fresh engine,
    before any copy is asked for.  The next run's outputs equal a fresh engine's."""
    two = [gc.Channel(p, dtype=2, f_if=0.0) for p in (3, 8)]
    three = [gc.Channel(p, dtype=2, f_if=0.0) for p in (3, 8, 15)]
    L = gc.lib()
    used, fresh = _engine(gc, noise, two), _engine(gc, noise, three)
    try:
        used.trk_set_state(_states(two, 45))
        used.trk_run(3)
        used.trk_fetch()
        used.set_channels(three)
        II, QQ = np.zeros((3, 3, 5)), np.zeros((3, 3, 5))
        ns = np.zeros((3, 3), np.int32)
        assert L.gnsscorr_trk_fetch(used.h, II.ctypes.data, QQ.ctypes.data, ns.ctypes.data) == ESTATE
        assert "no completed trk_run" in L.gnsscorr_last_error().decode()
        assert L.gnsscorr_trk_fetch_sums(used.h, II.ctypes.data, QQ.ctypes.data) == ESTATE
        assert "no completed trk_run" in L.gnsscorr_last_error().decode()
        with pytest.raises(gc.GnsscorrError, match="no completed trk_run"):
            used.trk_fetch()
        assert not II.any() and not QQ.any() and not ns.any()
        out = []
        for e in (used, fresh):
            e.trk_set_state(_states(three, 46))
            e.trk_run(3)
            out.append(list(e.trk_fetch()) + list(e.trk_fetch_sums()))
        _same(out[0], out[1], "after reconfiguration")
    finally:
        used.close()
        fresh.close()
