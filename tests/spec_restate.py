"""numpy restatement of the reference's IF monitor (test infrastructure, like oracle/): hanning(), calchistgram() and
spectrumanalyzer() of ref src/sdrspec.c, with the segment offsets passed in instead of drawn with rand().

The float inputs are formed exactly as the reference forms them; the transform is taken in complex128, so the only
difference to a correct fp32 FFT is that FFT's own rounding."""
import numpy as np

PI = 3.1415926535897932                 # ref src/sdr.h:103
SPEC_NLOOP = 100                        # ref src/sdr.h:232


def hanning(n):
    """ref src/sdrspec.c:214-219: (float)(0.5*(1-cos(2*PI*(i+1)/(n+1)))), the argument in double."""
    i = np.arange(n, dtype=np.float64)
    return (0.5 * (1 - np.cos(2 * PI * (i + 1) / (n + 1)))).astype(np.float32)


def calchistgram(data, dtype, n):
    """ref src/sdrspec.c:170-206 on n samples of int8 bytes `data` (interleaved I, Q for dtype 2).  Returns
    (yI, yQ) with 9 counts each: the reference's 8 bins and, at index 8, the count it writes one element past the
    end (d == maxd > 7)."""
    d = np.asarray(data, dtype=np.int8).reshape(-1).astype(np.int64)
    maxd = int(np.abs(d[:n * dtype]).max()) if n * dtype else 0          # :183
    yI = np.zeros(9, np.int64)
    yQ = np.zeros(9, np.int64)

    def bins(v):
        if maxd > 7:                                                     # (int)((double)d/maxd*4+4)
            return np.trunc(v.astype(np.float64) / maxd * 4 + 4).astype(np.int64)
        return np.trunc((v + 7) / 2).astype(np.int64)                    # C division: truncation

    if dtype == 1:                                                       # :186-192
        np.add.at(yI, bins(d[:n]), 1)
    else:                                                                # :193-205
        if maxd > 7:
            np.add.at(yI, bins(d[0:2 * n:2]), 1)
            np.add.at(yQ, bins(d[1:2 * n:2]), 1)
        else:                                                            # the reference indexes data[i], i < n, for both
            np.add.at(yI, bins(d[:n]), 1)
            np.add.at(yQ, bins(d[:n]), 1)
    return yI, yQ


def spec_inputs(data, dtype, nfft, nloop=SPEC_NLOOP):
    """x = (float)(data*(17.127/(nfft*2)/sqrt((float)nloop))) of ref src/sdrspec.c:254-255, as [n] or [n][2]."""
    d = np.asarray(data, dtype=np.int8).reshape(-1)
    scale = 17.127 / (nfft * 2) / np.sqrt(np.float64(np.float32(nloop)))
    x = (d.astype(np.float64) * scale).astype(np.float32)
    return x if dtype == 1 else x.reshape(-1, 2)


def spectrum_sums(data, dtype, nfft, offsets, nloop=None):
    """The reference's s[2*nfft] (ref src/sdrspec.c:257-278) for the segment offsets `offsets` (its zuz)."""
    nloop = len(offsets) if nloop is None else nloop
    nwin = nfft // 2
    win = hanning(nwin)
    x = spec_inputs(data, dtype, nfft, nloop)
    s = np.zeros(2 * nfft)
    for zuz in offsets:
        seg = np.zeros(2 * nfft, np.complex128)
        if dtype == 1:
            seg[:nwin] = win * x[zuz:zuz + nwin]                          # one fp32 multiply
        else:
            seg[:nwin] = (win * x[zuz:zuz + nwin, 0]).astype(np.float64) + 1j * (win * x[zuz:zuz + nwin, 1])
        X = np.fft.fft(seg)
        s += X.real ** 2 + X.imag ** 2
    return s


def spectrum_post(s, dtype, nfft, f_sf):
    """pspec (dB) and freq (MHz) from s, ref src/sdrspec.c:280-294, the same double expressions."""
    i = np.arange(dtype * nfft, dtype=np.float64)
    if dtype == 1:
        return 10 * np.log10(s[:nfft]), (i * (f_sf / 2) / (nfft)) / 1e6
    idx = (np.arange(2 * nfft) + nfft) % (2 * nfft)
    return 10 * np.log10(s[idx]), (-f_sf / 2 + i * f_sf / nfft / 2) / 1e6


def spectrumanalyzer(data, dtype, f_sf, nfft, offsets):
    """(freq, pspec, s) of ref src/sdrspec.c:232-296 with explicit offsets."""
    s = spectrum_sums(data, dtype, nfft, offsets)
    pspec, freq = spectrum_post(s, dtype, nfft, f_sf)
    return freq, pspec, s


def rand_offsets(rand_values, n, nfft, rand_max=2147483647):
    """zuz = (int)floor((double)rand()/RAND_MAX*maxshift), ref src/sdrspec.c:257 (glibc RAND_MAX)."""
    maxshift = n - nfft // 2
    return [int(np.floor(float(r) / rand_max * maxshift)) for r in rand_values]
