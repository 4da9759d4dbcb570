"""fec_viterbi27 on the GPU (-m gpu): gnsscorr_fec_run against the numpy restatement of the decoder (fec_restate.py).

Bar: every row of every window equals the restatement bit for bit -- the decoder is integer arithmetic with the tie
rule stated, so nothing is left to rounding."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fec_restate as fr  # noqa: E402
from test_fec_host import _codeword, spaced_errors  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = -1


def _full_windows():
    bits, clean = _codeword(1)
    bad = clean.copy()
    idx = spaced_errors(1)
    bad[idx] = -bad[idx]
    # a window whose true final state is not 0, and plain noise: no known answers, the restatement is the bar
    open_end = fr.encode(np.random.default_rng(8).integers(0, 2, size=756))
    noise = (1 - 2 * np.random.default_rng(9).integers(0, 2, size=fr.WIN)).astype(np.int8)
    one = np.ones(fr.WIN, np.int8)
    return bits, np.stack([clean, bad, one, -one, 0 * one, open_end, noise])


def test_full_window(engine):
    bits, sym = _full_windows()
    rows = engine.fec_run(sym, fr.WIN - 1, 1, rowbytes=fr.ROWBYTES)
    assert rows.shape == (7, 1, fr.ROWBYTES)
    ref = fr.fec_rows(sym, fr.WIN - 1, 1, rowbytes=fr.ROWBYTES)
    assert np.array_equal(rows, ref)
    for i in (0, 1):                                        # the two known answers, on the device's own rows
        assert np.array_equal(np.unpackbits(rows[i, 0])[:750], bits)
    assert not rows[:, :, 94:].any() and not (rows[:, 0, 93] & 3).any()


_STREAMS = {}


def _streams():
    """2 channels x 1812 symbols, a run of zeros at the front; and the restatement's rows for every position used."""
    if not _STREAMS:
        rng = np.random.default_rng(21)
        sym = (1 - 2 * rng.integers(0, 2, size=(2, 1812))).astype(np.int8)
        sym[0, :23] = 0
        sym[1, :70] = 0
        pos0 = fr.WIN - 1 - 40                              # the first 40 windows reach in front of the stream
        _STREAMS.update(sym=sym, pos0=pos0, ref=fr.fec_rows(sym, pos0, 301, rowbytes=fr.ROWBYTES))
    return _STREAMS


@pytest.mark.parametrize("npos", [1, 5, 301])
def test_sliding_windows_stride_1(engine, npos):
    s = _streams()
    rows = engine.fec_run(s["sym"], s["pos0"], npos, 1, rowbytes=fr.ROWBYTES)
    assert np.array_equal(rows, s["ref"][:, :npos])


def test_stride_500(engine):
    s = _streams()
    sym = np.concatenate([s["sym"], s["sym"][::-1]], axis=1)          # 3624 symbols: windows at 500-symbol steps
    pos0 = fr.WIN - 1 - 40
    for npos in (1, 5):
        rows = engine.fec_run(sym, pos0, npos, 500, rowbytes=fr.ROWBYTES)
        assert np.array_equal(rows, fr.fec_rows(sym, pos0, npos, 500, rowbytes=fr.ROWBYTES))
    assert pos0 + 4 * 500 == sym.shape[1] - 153


def test_small_generic_shape_and_swapped_polynomials(engine):
    rng = np.random.default_rng(22)
    sym = (1 - 2 * rng.integers(0, 2, size=(3, 190))).astype(np.int8)
    sym[2, :5] = 0
    a = engine.fec_run(sym, 20, 130, 1, win=44, ndec=16)
    b = engine.fec_run(sym, 20, 130, 1, win=44, ndec=16, polyA=fr.POLYB, polyB=fr.POLYA)
    assert a.shape == (3, 130, 2)
    assert np.array_equal(a, fr.fec_rows(sym, 20, 130, 1, 44, 16))
    assert np.array_equal(b, fr.fec_rows(sym, 20, 130, 1, 44, 16, fr.POLYB, fr.POLYA))
    assert not np.array_equal(a, b)
    c = engine.fec_run(sym, 20, 130, 1, win=44, ndec=13, rowbytes=5)  # bits that do not fill the byte, a padded row
    assert np.array_equal(c, fr.fec_rows(sym, 20, 130, 1, 44, 13, rowbytes=5))


def test_identical_bytes_whatever_memory_held(gc, engine):
    s = _streams()
    first = engine.fec_run(s["sym"], s["pos0"], 301, rowbytes=fr.ROWBYTES)
    assert np.array_equal(first, engine.fec_run(s["sym"], s["pos0"], 301, rowbytes=fr.ROWBYTES))
    for byte in (0x00, 0xFF, 0xA5):
        e = gc.Engine(0)
        try:
            e.debug_poison(byte)
            assert np.array_equal(first, e.fec_run(s["sym"], s["pos0"], 301, rowbytes=fr.ROWBYTES))
        finally:
            e.close()
    assert np.array_equal(first, s["ref"])


def test_timer_name(engine):
    engine.timing(1)
    engine.fec_run(_streams()["sym"], fr.WIN, 3, rowbytes=fr.ROWBYTES)
    ms, n = engine.timing_read("fec_viterbi27")
    assert n == 1 and ms > 0


def test_einval(gc, engine):
    L = gc.lib()
    sym = np.ones((1, 2000), np.int8)
    out = np.full(4 * 96, 0x5A, np.uint8)

    def run(nch=1, nsym=2000, pos0=1511, npos=4, stride=1, win=1512, ndec=750, rowbytes=96):
        return L.gnsscorr_fec_run(engine.h, sym.ctypes.data, nch, nsym, pos0, npos, stride, win, ndec, 0x6d, 0x4f,
                                  out.ctypes.data, rowbytes)

    assert run() == 0 and not (out == 0x5A).all()
    out[:] = 0x5A
    bad = [dict(win=1511), dict(win=1514), dict(ndec=751), dict(win=44, ndec=17), dict(rowbytes=93), dict(rowbytes=-1),
           dict(nch=-1), dict(nsym=-1), dict(pos0=-1), dict(npos=-1), dict(stride=-1), dict(ndec=-1),
           dict(pos0=1997), dict(stride=500)]
    for kw in bad:
        assert run(**kw) == EINVAL, kw
        assert gc.lib().gnsscorr_last_error()
    assert (out == 0x5A).all()                              # a failing call leaves its output untouched
    assert L.gnsscorr_fec_run(engine.h, None, 1, 2000, 1511, 4, 1, 1512, 750, 0x6d, 0x4f, out.ctypes.data, 96) == EINVAL
    assert run(npos=0) == 0 and (out == 0x5A).all()
