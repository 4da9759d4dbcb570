"""Engine lifecycle (-m gpu): every device buffer a context owns goes with it, and a channel set grown on a live
engine computes what a fresh engine computes.

The context owns its buffers through one owning type (gnsscorr_ctx.h): a create / use / destroy cycle that touches
every lazily made buffer (tracking at two batch lengths, the closed loop, acquisition, the IF monitor) must leave
the device's free memory where the first cycle left it."""
import ctypes as C

import numpy as np
import pytest

NSAMP = 16368


def _free_device_bytes(gc):
    # through the library's own handle: its symbol lookup reaches the HIP runtime libgnsscorr.so is linked against
    # (not torch's view of the device)
    hip = gc.lib()
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def _states(chans, seed):
    rng = np.random.default_rng(seed)
    return [dict(carrfreq=float(rng.uniform(-4000, 4000)), codefreq=c.crate + float(rng.uniform(-2, 2)),
                 remcode=float(rng.uniform(0.01, 0.99)), remcarr=float(rng.uniform(0, 6.2)), buffloc=100 + 900 * i)
            for i, c in enumerate(chans)]


def _cycle(gc, data, prns):
    n = data.shape[0]
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, n)
        eng.ring_push_raw(1, data, n)
        chans = [gc.Channel(p, dtype=2, f_if=0.0) for p in prns]
        eng.set_channels(chans)
        eng.trk_set_state(_states(chans, 7))
        eng.trk_run(20)
        eng.trk_fetch()
        eng.trk_run(50)                                 # a longer batch: the tracking buffers grow
        eng.trk_fetch()
        eng.trk_set_state(_states(chans, 8))
        eng.loop_set([eng.loop_state(i, 1000.0) for i in range(len(chans))])
        eng.trk_run_loop(10)
        eng.trk_fetch_log()
        eng.acq_run()
        eng.acq_fetch()
        eng.spectrum(1, 0, 4 * NSAMP, 16.368e6, seed=3)
        eng.sync()
    finally:
        eng.close()


@pytest.mark.gpu
def test_create_use_destroy_cycles_return_device_memory(gc):
    rng = np.random.default_rng(11)
    n = NSAMP * 80
    data = rng.integers(-60, 61, size=(n, 2), dtype=np.int8)
    free = []
    for _ in range(3):
        _cycle(gc, data, (1, 5, 9, 13))
        free.append(_free_device_bytes(gc))
    print("free device bytes after cycles 1..3:", free, "drift", free[0] - free[2])
    # no slack: on MI355X the three readings were identical to the byte, so any leaked device buffer the runtime
    # accounts for fails this.  (Pinned host memory is not visible here.)
    assert free[2] == free[1] and free[2] >= free[0], free


def _batches(eng, states, lengths):
    """Batches of the given lengths from one state (a repeated length runs on the look-ahead plan)."""
    eng.trk_set_state(states)
    out = []
    for nepoch in lengths:
        eng.trk_run(nepoch)
        out.extend(eng.trk_fetch())
    return out, eng.trk_get_state()


@pytest.mark.gpu
def test_set_channels_grown_on_a_live_engine_matches_a_fresh_engine(gc):
    rng = np.random.default_rng(12)
    n = NSAMP * 200
    data = rng.integers(-60, 61, size=(n, 2), dtype=np.int8)
    small = [gc.Channel(p, dtype=2, f_if=0.0) for p in (3, 4)]
    big = [gc.Channel(p, dtype=2, f_if=0.0, corrn=3, corrd=3, corrp=3) for p in (2, 7, 11, 17, 23, 29)]
    live, fresh = gc.Engine(0), gc.Engine(0)
    try:
        for e in (live, fresh):
            e.ring_create(1, 2, n)
            e.ring_push_raw(1, data, n)
        # the live engine first runs a smaller channel set: batches of two lengths, the closed loop, acquisition
        live.set_channels(small)
        _batches(live, _states(small, 22), (30, 60))
        live.trk_set_state(_states(small, 23))
        live.loop_set([live.loop_state(i, 500.0) for i in range(len(small))])
        live.trk_run_loop(8)
        live.acq_run()
        live.acq_fetch()
        live.set_channels(big)                          # more channels, more taps: every buffer must grow
        fresh.set_channels(big)
        a, sa = _batches(live, _states(big, 21), (40, 40, 90))
        b, sb = _batches(fresh, _states(big, 21), (40, 40, 90))
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), k
        assert sa == sb
    finally:
        live.close()
        fresh.close()
