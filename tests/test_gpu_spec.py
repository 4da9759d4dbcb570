"""IF monitor on the GPU (-m gpu): gnsscorr_spec_run/fetch on the HBM ring and the spectrumanalyzer() drop-in,
against the numpy restatement in spec_restate.py.

Bars: frequency axis and histogram counts bit-exact; linear sums within rel_err 1e-5 (the bar of
test_cpxfft_cpxpspec_any_length: only the fp32 FFT's rounding differs, the inputs are the reference's floats);
dB within 1e-3 on every bin at least 1e-4 of the peak; the device results bit-identical from run to run, from
batch to single snapshot, and whatever scratch memory held before."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spec_restate as sr  # noqa: E402
from conftest import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

F_SF = 16.368e6
EINVAL = -1


def _libc():
    return C.CDLL("libc.so.6")


# ---- 1. the drop-in ----------------------------------------------------------------------------------------------
DROPIN = [(d, n, nfft) for d in (1, 2) for n in (7 * 16368, 7 * 20000) for nfft in (16384, 8192)] + \
         [(2, 7 * 16368, 1000), (1, 5000, 1000)]


@pytest.mark.parametrize("dtype,n,nfft", DROPIN, ids=[f"d{d}_n{n}_nfft{f}" for d, n, f in DROPIN])
def test_spectrumanalyzer_dropin_parity(gc, dtype, n, nfft):
    rng = np.random.default_rng(n + nfft + dtype)
    data = np.clip(np.rint(rng.normal(0, 8, size=n * dtype)), -127, 127).astype(np.int8)
    gc.spectrumanalyzer(data, dtype, F_SF, nfft)             # the device is up before the seeded call
    libc, seed = _libc(), 1234 + n % 97
    libc.srand(seed)
    freq, pspec = gc.spectrumanalyzer(data, dtype, F_SF, nfft)
    libc.srand(seed)
    offs = sr.rand_offsets([libc.rand() for _ in range(sr.SPEC_NLOOP)], n, nfft)
    freq_r, pspec_r, s_r = sr.spectrumanalyzer(data, dtype, F_SF, nfft, offs)
    assert freq.size == pspec.size == dtype * nfft
    assert np.array_equal(freq, freq_r)
    s_lin = 10.0 ** (pspec / 10)
    s_lin_r = 10.0 ** (pspec_r / 10)
    assert rel_err(s_lin, s_lin_r) < 1e-5
    big = s_lin_r >= 1e-4 * s_lin_r.max()
    assert np.abs(pspec - pspec_r)[big].max() < 1e-3


# ---- 2. the ring API ---------------------------------------------------------------------------------------------
N = 7 * 16368
RINGLEN = 3 * N                        # dtype*ringlen a multiple of 16 for both dtypes


def _stereo_engine(gc, seed=5, poison=None):
    """Rings 1 (real) and 2 (IQ) fed by NSL Stereo bytes until both have wrapped."""
    e = gc.Engine(0)
    if poison is not None:
        e.debug_poison(poison)
    e.ring_create(1, 1, RINGLEN)
    e.ring_create(2, 2, RINGLEN)
    packed = np.random.default_rng(seed).integers(0, 256, size=4 * N + 12345, dtype=np.uint8)
    half = packed.size // 2
    e.ring_push_packed(gc.FMT_STEREO, packed[:half], half)
    e.ring_push_packed(gc.FMT_STEREO, packed[half:], packed.size - half)
    return e


def _snapshots(wrpos, nfft, nsnap=8, nloop=100, seed=3):
    rng = np.random.default_rng(seed)
    oldest, last = wrpos - RINGLEN, wrpos - N
    wrap = (wrpos // RINGLEN) * RINGLEN - 1000           # crosses the ring end
    assert oldest <= wrap <= last
    locs = [wrap, oldest, last] + [int(v) for v in rng.integers(oldest, last + 1, size=nsnap - 3)]
    offs = rng.integers(0, N - nfft // 2 + 1, size=(nsnap, nloop)).astype(np.int32)
    offs[:, 0] = 0
    offs[:, 1] = N - nfft // 2
    return np.array(locs, np.uint64), offs


def _restated(eng, ftype, dtype, loc, offs, nfft):
    data = eng.ring_read(ftype, int(loc), N, dtype)
    freq, pspec, s = sr.spectrumanalyzer(data, dtype, F_SF, nfft, list(offs))
    yI, yQ = sr.calchistgram(data, dtype, N)
    return freq, pspec, s, np.stack([yI, yQ])


def _assert_vs_restatement(eng, ftype, dtype, nfft, locs, offs, freq, pspec, s, hist):
    for k in range(len(locs)):
        freq_r, pspec_r, s_r, hist_r = _restated(eng, ftype, dtype, locs[k], offs[k], nfft)
        assert np.array_equal(freq, freq_r)
        assert rel_err(s[k], s_r) < 1e-5, k
        lin = np.empty(dtype * nfft)
        lin[:] = s_r[:nfft] if dtype == 1 else s_r[(np.arange(2 * nfft) + nfft) % (2 * nfft)]
        big = lin >= 1e-4 * lin.max()
        assert np.abs(pspec[k] - pspec_r)[big].max() < 1e-3, k
        assert np.array_equal(hist[k], hist_r), k
        assert hist[k, 0].sum() == N
        assert hist[k, 1].sum() == (N if dtype == 2 else 0)


@pytest.mark.parametrize("ftype,dtype,nfft", [(1, 1, 16384), (2, 2, 16384), (2, 2, 8192), (1, 1, 8192)])
def test_ring_spectrum_batch_single_and_restatement(gc, ftype, dtype, nfft):
    eng = _stereo_engine(gc)
    try:
        locs, offs = _snapshots(eng.ring_wrpos(ftype), nfft)
        freq, pspec, s, hist = eng.spectrum(ftype, locs, N, F_SF, nfft=nfft, offsets=offs)
        assert pspec.shape == (8, dtype * nfft) and s.shape == (8, 2 * nfft) and hist.shape == (8, 2, 9)
        for k in range(8):
            f1, p1, s1, h1 = eng.spectrum(ftype, int(locs[k]), N, F_SF, nfft=nfft, offsets=offs[k:k + 1])
            assert np.array_equal(f1, freq)
            assert np.array_equal(s1, s[k]) and np.array_equal(p1, pspec[k]) and np.array_equal(h1, hist[k])
        _assert_vs_restatement(eng, ftype, dtype, nfft, locs, offs, freq, pspec, s, hist)
        assert hist[:, :, 8].sum() == 0                   # Stereo levels stay within 3 bits: maxd <= 7
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", [1, 2])
def test_ring_histogram_wide_samples(gc, dtype):
    """int8 samples (maxd > 7: the scaled bins, bin 8 for d == maxd), one snapshot across the ring end."""
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, dtype, RINGLEN)
        rng = np.random.default_rng(11)
        nsamp = RINGLEN + N
        data = rng.integers(-90, 91, size=(nsamp, 2) if dtype == 2 else nsamp).astype(np.int8)
        flat = data.reshape(-1)
        flat[rng.integers(0, flat.size, 50)] = 101        # maxd, several times (I and Q)
        flat[rng.integers(0, flat.size, 50)] = -101
        eng.ring_push_raw(1, data[:RINGLEN], RINGLEN)
        eng.ring_push_raw(1, data[RINGLEN:], N)
        wr = eng.ring_wrpos(1)
        locs = np.array([RINGLEN - 777, wr - N, wr - RINGLEN], np.uint64)
        offs = np.random.default_rng(2).integers(0, N - 8192 + 1, size=(3, 100)).astype(np.int32)
        freq, pspec, s, hist = eng.spectrum(1, locs, N, F_SF, nfft=16384, offsets=offs)
        _assert_vs_restatement(eng, 1, dtype, 16384, locs, offs, freq, pspec, s, hist)
        assert hist[:, 0, 8].sum() > 0
    finally:
        eng.close()


# ---- 3. determinism ----------------------------------------------------------------------------------------------
def test_spectrum_deterministic_and_independent_of_scratch(gc):
    eng = _stereo_engine(gc)
    locs, offs = _snapshots(eng.ring_wrpos(2), 16384)
    try:
        a = eng.spectrum(2, locs, N, F_SF, offsets=offs)
        b = eng.spectrum(2, locs, N, F_SF, offsets=offs)
    finally:
        eng.close()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    eng = _stereo_engine(gc, poison=0xA5)
    try:
        c = eng.spectrum(2, locs, N, F_SF, offsets=offs)
    finally:
        eng.close()
    for x, y in zip(a, c):
        assert np.array_equal(x, y)


# ---- 4. no interference ------------------------------------------------------------------------------------------
def _tracking_run(gc, with_spectrum):
    nsamp = 16368
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, 200 * nsamp)
        data = np.random.default_rng(21).integers(-60, 61, size=(150 * nsamp, 2), dtype=np.int8)
        eng.ring_push_raw(1, data, 150 * nsamp)
        chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3) for p in range(1, 33)]
        eng.set_channels(chans)
        rng = np.random.default_rng(22)
        eng.trk_set_state([dict(carrfreq=float(rng.uniform(-5000, 5000)), codefreq=c.crate + float(rng.uniform(-3, 3)),
                                remcode=float(rng.uniform(0, 1)), remcarr=float(rng.uniform(0, 6.2)),
                                buffloc=int(rng.integers(0, nsamp))) for c in chans])
        out, specs = [], []
        for b in range(4):
            if with_spectrum:
                specs.append(eng.spectrum(1, [150 * nsamp - N - 1000 * b, 5000], N, F_SF, seed=b))
            eng.trk_run(10)
            if with_spectrum:
                specs.append(eng.spectrum(1, 150 * nsamp - N, N, F_SF, nfft=8192, seed=b))
            out.append(eng.trk_fetch())
        return out, specs
    finally:
        eng.close()


def test_spectrum_between_tracking_batches(gc):
    base, _ = _tracking_run(gc, False)
    mixed, specs = _tracking_run(gc, True)
    assert len(specs) == 8
    for (I0, Q0, n0), (I1, Q1, n1) in zip(base, mixed):
        assert np.array_equal(I0, I1) and np.array_equal(Q0, Q1) and np.array_equal(n0, n1)


def test_acquisition_unchanged_by_spectrum(gc, synth):
    eng = gc.Engine(0)
    try:
        chans = [gc.Channel(p, dtype=2, f_if=0.0) for p in (3, 11, 19, 27)]
        codes = {c.prn: (c.code, c.crate) for c in chans}
        nsamp = 12 * chans[0].nsamp
        data = synth.make_if(codes, nsamp, dtype=2,
                             sats=[dict(prn=11, doppler=1300.0, codephase=200.5, cn0=47.0)], seed=4)
        eng.ring_create(1, 2, nsamp)
        eng.ring_push(1, data)
        eng.set_channels(chans)
        eng.acq_run()
        before = eng.acq_fetch()
        eng.spectrum(1, nsamp - N, N, F_SF, seed=1)
        eng.acq_run()
        after = eng.acq_fetch()
        assert before == after
    finally:
        eng.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------------
def test_spectrum_errors_write_nothing(gc):
    L = gc.lib()
    eng = _stereo_engine(gc)
    try:
        wr = eng.ring_wrpos(2)
        ok_locs, ok_offs = _snapshots(wr, 16384, nsnap=4, nloop=10)
        ref = eng.spectrum(2, ok_locs, N, F_SF, nloop=10, offsets=ok_offs)

        def run(locs, offs, nfft=16384, nloop=10):
            sp = gc.SpecParams(2, nfft, nloop, N, F_SF)
            locs = np.ascontiguousarray(locs, np.uint64)
            offs = np.ascontiguousarray(offs, np.int32)
            return L.gnsscorr_spec_run(eng.h, C.byref(sp), len(locs), locs.ctypes.data, offs.ctypes.data)

        def fetch_equal_to_ref():
            s = np.empty_like(ref[2]); p = np.empty_like(ref[1]); f = np.empty_like(ref[0])
            h = np.empty(ref[3].shape, np.int64)
            assert L.gnsscorr_spec_fetch(eng.h, s.ctypes.data, s.size, p.ctypes.data, p.size, f.ctypes.data, f.size,
                                         h.ctypes.data, h.size) == 0
            return np.array_equal(s, ref[2]) and np.array_equal(p, ref[1]) and np.array_equal(h, ref[3])

        cases = []
        bad = ok_locs.copy(); bad[1] = wr - RINGLEN - 1                  # already overwritten
        cases.append((bad, ok_offs, 16384, "snapshot 1"))
        bad = ok_locs.copy(); bad[2] = wr - N + 1                        # runs past wrpos
        cases.append((bad, ok_offs, 16384, "snapshot 2"))
        bad = ok_offs.copy(); bad[3, 4] = N - 8192 + 1                   # offset past n - nfft/2
        cases.append((ok_locs, bad, 16384, "snapshot 3"))
        bad = ok_offs.copy(); bad[0, 9] = -1
        cases.append((ok_locs, bad, 16384, "snapshot 0"))
        cases.append((ok_locs, ok_offs, 4096, "nfft"))                   # unsupported transform
        for locs, offs, nfft, msg in cases:
            assert run(locs, offs, nfft) == EINVAL, msg
            assert msg in L.gnsscorr_last_error().decode()
            assert fetch_equal_to_ref(), msg                             # nothing launched: the last run stands
        # a fetch capacity one element short: EINVAL, the array untouched
        nsnap, dtype, nfft = 4, 2, 16384
        need = {"s": nsnap * 2 * nfft, "p": nsnap * dtype * nfft, "f": dtype * nfft, "h": nsnap * 18}
        for which in need:
            bufs = {k: np.full(v, 7.0) if k != "h" else np.full(v, 7, np.int64) for k, v in need.items()}
            caps = dict(need)
            caps[which] -= 1
            rc = L.gnsscorr_spec_fetch(eng.h, bufs["s"].ctypes.data, caps["s"], bufs["p"].ctypes.data, caps["p"],
                                       bufs["f"].ctypes.data, caps["f"], bufs["h"].ctypes.data, caps["h"])
            assert rc == EINVAL, which
            for b in bufs.values():
                assert np.all(b == 7), which
        assert fetch_equal_to_ref()
    finally:
        eng.close()


# ---- 6. physics --------------------------------------------------------------------------------------------------
def test_cw_interferer_on_a_flat_floor(gc, synth):
    nfft = 16384
    chans = [gc.Channel(p, dtype=2, f_if=0.0) for p in (5, 12)]
    codes = {c.prn: (c.code, c.crate) for c in chans}
    nsamp = 2 * N
    data = synth.make_if(codes, nsamp, dtype=2, seed=9,
                         sats=[dict(prn=5, doppler=-2100.0, codephase=10.0, cn0=45.0),
                               dict(prn=12, doppler=3300.0, codephase=700.0, cn0=42.0)]).astype(np.float64)
    m = 2473                                                    # interferer on FFT bin m: +1.2355 MHz
    f_cw = m * F_SF / (2 * nfft)
    t = np.arange(nsamp) / F_SF
    data[:, 0] += 6.0 * np.cos(2 * np.pi * f_cw * t)            # exp(+i 2 pi f t)
    data[:, 1] += 6.0 * np.sin(2 * np.pi * f_cw * t)
    iq = np.clip(np.rint(data), -127, 127).astype(np.int8)
    eng = gc.Engine(0)
    try:
        eng.ring_create(1, 2, nsamp)
        eng.ring_push(1, iq)
        freq, pspec, s, hist = eng.spectrum(1, nsamp - N, N, F_SF, nfft=nfft, seed=0)
    finally:
        eng.close()
    k = int(np.argmax(pspec))
    assert abs(freq[k] - f_cw / 1e6) < 1e-9
    rest = np.delete(pspec, np.arange(k - 64, k + 65))
    floor = np.median(rest)
    assert pspec[k] - floor > 20
    # 100 Hann segments drawn from 8 windows' worth of samples: the floor's bins scatter by ~1 dB
    assert np.percentile(np.abs(rest - floor), 99) < 3.0
    assert np.abs(rest - floor).max() < 7.0
    assert hist[0].sum() == N and hist[1].sum() == N
