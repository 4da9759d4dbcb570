"""Acquisition's host driver (gnsscorr_acq.hip, below the kernels) and what the context keeps for it: the FFT tables
for the context's lifetime (GcFftTables), the search state per channel set and coherent setting (GcAcq), the IF
monitor's per channel set (GcSpec), and the streams and events the context makes on first use.

Every comparison is exact equality with a fresh engine's bytes or with an error code: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_lifecycle import _free_device_bytes

pytestmark = pytest.mark.gpu
ESTATE = -3
RING = 80000                    # IQ samples: the longest search here looks (intg + 1) * 20000 = 60000 back
GRID = dict(hband=400, step=200, intg=2)         # 5 Doppler bins, 2 code periods


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(71).integers(-60, 61, size=(RING, 2), dtype=np.int8)


def _set32k(gc, ncoh=(1, 1)):
    """The 32768-point transform: 4092 samples per code period."""
    return [gc.Channel(p, dtype=2, f_if=0.0, f_sf=4.092e6, ncoh=k, **GRID) for p, k in zip((3, 19), ncoh)]


def _set64k(gc):
    """The 65536-point transform: 20000 samples per code period."""
    return [gc.Channel(p, dtype=2, f_if=0.0, f_sf=20e6, **GRID) for p in (7, 22)]


def _engine(gc, data, chans=None):
    e = gc.Engine(0)
    e.ring_create(1, 2, RING)
    e.ring_push_raw(1, data, RING)
    if chans:
        e.set_channels(chans)
    return e


def _search(gc, eng):
    """One search over every channel: the result rows (every field of every gnsscorr_acqres_t) and channel 0's power
    array, as bytes."""
    eng.acq_run()
    res = (gc.AcqRes * len(eng.channels))()
    assert gc.lib().gnsscorr_acq_fetch(eng.h, res) == 0
    P = eng.acq_power(0)
    assert P.any()
    return bytes(res), P.tobytes()


def _acq_calls(gc, eng):
    """The return codes and messages of the four calls that need a search's results."""
    L = gc.lib()
    nch = len(eng.channels)
    res = (gc.AcqRes * nch)()
    P = np.zeros((eng.channels[0].nfreq, eng.channels[0].nsamp))
    out = []
    for call in (lambda: L.gnsscorr_acq_fetch(eng.h, res), lambda: L.gnsscorr_acq_power(eng.h, 0, P.ctypes.data),
                 lambda: L.gnsscorr_trk_start_from_acq(eng.h), lambda: L.gnsscorr_loop_start_from_acq(eng.h)):
        out.append((call(), L.gnsscorr_last_error().decode()))
    assert not bytes(res).strip(b"\0") and not P.any()
    return out


def _spec_fetch(gc, eng):
    L = gc.lib()
    freq = np.zeros(2 * 8192)
    return L.gnsscorr_spec_fetch(eng.h, None, 0, None, 0, freq.ctypes.data, freq.size, None, 0), L.gnsscorr_last_error().decode()


def test_fetches_after_reconfiguration(gc, noise):
    """An engine that has searched and run the IF monitor answers GNSSCORR_ESTATE to every fetch after set_channels,
    and to the four acquisition calls after acq_set_coherent, exactly as an engine that never ran either."""
    used, fresh = _engine(gc, noise, _set32k(gc)), _engine(gc, noise, _set32k(gc))
    try:
        want = _acq_calls(gc, fresh)
        assert [rc for rc, _ in want] == [ESTATE] * 4
        assert all("no acq_run yet" in msg for _, msg in want)
        want_spec = _spec_fetch(gc, fresh)
        assert want_spec[0] == ESTATE and "no spec_run yet" in want_spec[1]

        _search(gc, used)
        used.spectrum(1, 1000, 20000, 4.092e6, nfft=8192, nloop=4, seed=1)
        assert _spec_fetch(gc, used)[0] == 0
        used.set_channels(_set32k(gc))
        assert _acq_calls(gc, used) == want
        assert _spec_fetch(gc, used) == want_spec

        _search(gc, used)
        used.acq_set_coherent([2, 1])
        assert _acq_calls(gc, used) == want
    finally:
        used.close()
        fresh.close()


def test_search_on_a_reconfigured_engine_equals_a_fresh_engine(gc, noise):
    """One live engine goes through a 32768-point set, a 65536-point set (X and C grow, L changes), the first set
    again, and the first set with two periods integrated coherently on channel 1 (acq_set_coherent on the engine that
    has just searched).  After each step its results and channel 0's power array equal a fresh engine's."""
    steps = [("32k", _set32k(gc)), ("64k", _set64k(gc)), ("32k again", _set32k(gc)), ("ncoh 2", _set32k(gc, (1, 2)))]
    live = _engine(gc, noise)
    try:
        seen = []
        for what, chans in steps:
            if what == "ncoh 2":
                live.acq_set_coherent([c.ncoh for c in chans])
            else:
                live.set_channels(chans)
            assert live.acq_get_coherent() == [c.ncoh for c in chans], what
            fresh = _engine(gc, noise, chans)
            try:
                a, b = _search(gc, live), _search(gc, fresh)
            finally:
                fresh.close()
            assert a[0] == b[0], what
            assert a[1] == b[1], what
            seen.append(a)
        assert seen[0] == seen[2]                       # the same set, the same ring
        assert seen[0][0] != seen[3][0]                 # the coherent setting reached the search
    finally:
        live.close()


class _DevMem:
    """Device memory through the HIP runtime the library is linked against."""

    def __init__(self, gc, nbytes):
        self.hip, self.p = gc.lib(), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(nbytes)) == 0

    def put(self, a):
        assert self.hip.hipMemcpy(self.p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0

    def get(self, a):
        assert self.hip.hipMemcpy(C.c_void_p(a.ctypes.data), self.p, C.c_size_t(a.nbytes), 2) == 0
        return a

    def free(self):
        assert self.hip.hipFree(self.p) == 0


def _transforms(gc, eng, x, din, dout):
    """gnsscorr_fft16k (batch 1) with both signs and gnsscorr_pspec (16384 points) of x, as bytes."""
    L = gc.lib()
    out = []
    for sign in (-1, +1):
        assert L.gnsscorr_fft16k(eng.h, din.p, dout.p, sign, 1) == 0
        eng.sync()
        y = dout.get(np.zeros(16384, np.complex64))
        assert y.any()
        out.append(y.tobytes())
    ps = np.zeros(16384)
    assert L.gnsscorr_pspec(eng.h, x.ctypes.data, 16384, 0, ps.ctypes.data) == 0
    assert ps.any()
    out.append(ps.tobytes())
    return out


def test_fft_tables_outlive_channel_sets(gc, noise):
    """The transforms give the same bytes on an engine with no channels, after set_channels, and after a search and a
    second set_channels; a search after all of that equals a fresh engine's."""
    rng = np.random.default_rng(72)
    x = (rng.standard_normal(16384) + 1j * rng.standard_normal(16384)).astype(np.complex64)
    din, dout = _DevMem(gc, x.nbytes), _DevMem(gc, x.nbytes)
    eng, fresh = gc.Engine(0), None
    try:
        din.put(x)
        first = _transforms(gc, eng, x, din, dout)
        eng.ring_create(1, 2, RING)
        eng.ring_push_raw(1, noise, RING)
        eng.set_channels(_set32k(gc))
        assert _transforms(gc, eng, x, din, dout) == first
        _search(gc, eng)
        eng.set_channels(_set32k(gc))
        assert _transforms(gc, eng, x, din, dout) == first
        fresh = _engine(gc, noise, _set32k(gc))
        assert _search(gc, eng) == _search(gc, fresh)
    finally:
        eng.close()
        if fresh:
            fresh.close()
        din.free()
        dout.free()


def _lazy_cycle(gc, data, din, dout):
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, RING)
        eng.ring_push_raw(1, data, RING)                                    # the ingest stream and its events
        eng.ring_push_packed(gc.FMT_RTLSDR, data.view(np.uint8), RING)      # the device staging of the packed formats
        eng.set_channels(_set32k(gc))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(2)])
        eng.rx_start()
        eng.rx_lock_set(dict(sync_periods=2600, kbits=10, nbad=2, mu_min=5.0), ch0=0, nch=1)    # the lock event
        eng.timing(True)
        assert gc.lib().gnsscorr_fft16k(eng.h, din.p, dout.p, -1, 1) == 0   # leaves a pending pair of timer events
        eng.sync()
    finally:
        eng.close()


def test_create_destroy_cycles_with_lazy_handles_return_device_memory(gc, noise):
    """Three create / destroy cycles that make every handle the context makes on first use.  Free device memory shows
    leaked buffers only: a leaked event or stream is not visible here, so for the handles this holds the destroy path
    to completing, and to freeing the buffers that sit beside them (staging, FFT tables)."""
    x = np.ones(16384, np.complex64)
    din, dout = _DevMem(gc, x.nbytes), _DevMem(gc, x.nbytes)
    try:
        din.put(x)
        free = []
        for _ in range(3):
            _lazy_cycle(gc, noise, din, dout)
            free.append(_free_device_bytes(gc))
        print("free device bytes after cycles 1..3:", free)
        assert free[2] == free[1] and free[2] >= free[0], free
    finally:
        din.free()
        dout.free()
