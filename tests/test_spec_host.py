"""IF monitor, host side (no GPU): the hanning() and calchistgram() drop-ins against the restatement in
spec_restate.py, the restatement against physics, and spectrumanalyzer()'s refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spec_restate as sr  # noqa: E402


@pytest.mark.parametrize("n", [1, 8192])
def test_hanning_dropin_bit_exact(gc, n):
    w = np.zeros(n, np.float32)
    gc.lib().hanning(n, w.ctypes.data)
    i = np.arange(n, dtype=np.float64)
    closed = (0.5 * (1 - np.cos(2 * np.pi * (i + 1) / (n + 1)))).astype(np.float32)
    assert np.array_equal(w.view(np.uint32), closed.view(np.uint32))
    assert np.array_equal(sr.hanning(n).view(np.uint32), closed.view(np.uint32))


def _dropin_hist(gc, data, dtype, n):
    xI, yI, xQ, yQ = gc.calchistgram(data, dtype)
    assert np.array_equal(xI, [-7, -5, -3, -1, 1, 3, 5, 7]) and np.array_equal(xQ, xI)
    return yI, yQ


def _cases():
    rng = np.random.default_rng(7)
    r1 = rng.integers(-40, 41, size=5001).astype(np.int8)
    r1[17] = 53                                                 # maxd = 53, present once: bin 8
    r2 = rng.integers(-90, 91, size=(4000, 2)).astype(np.int8)
    r2[5, 1] = -100                                             # maxd on Q, negative: bin 0, no bin 8 on Q
    r2[9, 0] = 100                                              # ... and +maxd on I: bin 8
    two = rng.choice(np.array([-3, -1, 1, 3], np.int8), size=(3000, 2))
    three = rng.choice(np.array([-7, -5, -3, -1, 1, 3, 5, 7], np.int8), size=3001)
    three2 = np.stack([rng.choice(np.array([-7, -5, -3, -1, 1, 3, 5, 7], np.int8), size=2500),
                       rng.choice(np.array([-3, -1, 1, 3], np.int8), size=2500)], axis=1)
    return [("int8_real", r1, 1), ("int8_iq", r2, 2), ("2bit_iq", two, 2), ("3bit_real", three, 1),
            ("3bit_iq", three2, 2), ("zero_real", np.zeros(100, np.int8), 1), ("zero_iq", np.zeros((64, 2), np.int8), 2)]


@pytest.mark.parametrize("name,data,dtype", _cases(), ids=[c[0] for c in _cases()])
def test_calchistgram_dropin_vs_restatement(gc, name, data, dtype):
    n = data.size // dtype
    yI, yQ = _dropin_hist(gc, data, dtype, n)
    rI, rQ = sr.calchistgram(data, dtype, n)
    assert np.array_equal(yI, rI[:8]) and np.array_equal(yQ, rQ[:8])
    flat = data.reshape(-1).astype(np.int64)
    maxd = np.abs(flat).max()
    if maxd > 7:
        # bin 8 counts exactly the samples equal to +maxd; the drop-in leaves it out, so its bins sum short of n
        if dtype == 1:
            assert rI[8] == np.count_nonzero(flat == maxd) and rI[8] > 0
        else:
            assert rI[8] == np.count_nonzero(flat[0::2] == maxd) and rI[8] > 0
            assert rQ[8] == np.count_nonzero(flat[1::2] == maxd)
        assert yI.sum() == n - rI[8]
    else:
        assert rI[8] == 0 and yI.sum() == n
        if dtype == 2:
            # the quirk: both rows count data[i], i < n -- the first n interleaved bytes, not the Q samples
            assert np.array_equal(yQ, yI)
            assert np.array_equal(rI[:8], np.bincount((flat[:n] + 7) // 2, minlength=8))
    if name.startswith("zero"):
        assert yI[3] == n and yI.sum() == n


@pytest.mark.parametrize("dtype", [1, 2])
def test_restatement_tone_peaks_at_its_frequency(dtype):
    f_sf, nfft, m = 16.368e6, 1024, 173
    f0 = m * f_sf / (2 * nfft)                                  # bin-centred in the 2*nfft transform
    n = 4 * nfft
    t = np.arange(n) / f_sf
    if dtype == 1:
        data = np.rint(60 * np.cos(2 * np.pi * f0 * t)).astype(np.int8)
    else:
        data = np.stack([np.rint(60 * np.cos(2 * np.pi * f0 * t)), np.rint(60 * np.sin(2 * np.pi * f0 * t))],
                        axis=1).astype(np.int8)
    freq, pspec, s = sr.spectrumanalyzer(data, dtype, f_sf, nfft, [0, 100, 2000, n - nfft // 2])
    k = int(np.argmax(pspec))
    assert abs(freq[k] - f0 / 1e6) < 1e-12
    assert pspec[k] - np.median(pspec) > 40
    if dtype == 2:                                              # the negative frequency holds no tone
        kneg = int(np.argmin(np.abs(freq + f0 / 1e6)))
        assert pspec[k] - pspec[kneg] > 40


def test_restatement_frequency_axis_endpoints():
    f_sf, nfft = 16.368e6, 16384
    _, f1 = sr.spectrum_post(np.ones(2 * nfft), 1, nfft, f_sf)
    _, f2 = sr.spectrum_post(np.ones(2 * nfft), 2, nfft, f_sf)
    assert f1.size == nfft and f1[0] == 0.0 and f1[-1] == ((nfft - 1) * (f_sf / 2) / nfft) / 1e6
    assert f2.size == 2 * nfft and f2[0] == (-f_sf / 2) / 1e6 and f2[nfft] == 0.0
    assert f2[-1] == (-f_sf / 2 + (2 * nfft - 1) * f_sf / nfft / 2) / 1e6
    assert np.allclose(np.diff(f2), f_sf / (2 * nfft) / 1e6, rtol=1e-9, atol=0)


def test_spectrumanalyzer_refuses_short_input(gc):
    """n < nfft/2 is -1 before any device is touched (the reference would read before its buffer)."""
    L = gc.lib()
    data = np.zeros(100, np.int8)
    freq, pspec = np.full(2, 7.0), np.full(2, 7.0)
    assert L.spectrumanalyzer(data.ctypes.data, 1, 100, 16.368e6, 16384, freq.ctypes.data, pspec.ctypes.data) == -1
    assert "nfft/2" in L.gnsscorr_last_error().decode()
    assert np.all(freq == 7.0) and np.all(pspec == 7.0)


def test_spectrumanalyzer_no_device_fails_loudly(gc):
    """No CPU fallback: without a GPU, spectrumanalyzer returns -1 and says why."""
    L = gc.lib()
    if L.gnsscorr_device_count() > 0:
        pytest.skip("a GPU is visible here")
    data = np.ones(20000, np.int8)
    freq, pspec = np.zeros(16384), np.zeros(16384)
    assert L.spectrumanalyzer(data.ctypes.data, 1, 20000, 16.368e6, 16384, freq.ctypes.data, pspec.ctypes.data) == -1
    assert "device" in L.gnsscorr_last_error().decode()
    with pytest.raises(gc.GnsscorrError, match="device"):
        gc.spectrumanalyzer(data, 1, 16.368e6)
