"""The carrier chain's staged records (csrc/gnsscorr_nco.h: gc_car_rec_make, gc_carrier_rec_step_one,
gc_one_binade_consts) on the CPU: 300-period chains taken period by period the way the batch planner's carrier
wavefront takes them -- bracket discovered around an estimate of the start, (row, n) turned into a record, the step
chosen from the record -- against the oracle's literal mixcarr loop, bit for bit in every period.

The one-binade step on a record must agree with the reference form (gc_carrier_value_step_one) wherever both step,
and must never step where the reference form does not.  So that the chains cannot pass on fallbacks, the share of
periods served by the record's own steps is asserted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "nco_rec_host.cpp")
DPI = 2.0 * 3.1415926535897932
NPER = 300
W0 = 2.0 ** -30


@pytest.fixture(scope="module")
def ncr(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ncr") / "nco_rec_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    d, i, vp = C.c_double, C.c_int, C.c_void_p
    L.ncr_period.argtypes = [d, i, d, i, d, d, i, vp, vp, vp]
    L.ncr_consts.argtypes = [d, d, i]
    return L


def _chain(ncr, orc, freq, f_sf, remcarr, rng, nper=NPER, est_err=1e-11, wide_miss=0, nrow_off=0):
    """-> how[nper]; asserts every period against the oracle.  est_err: how far the discovery's estimate lies from
    the exact start (fraction of the bracket's width is what matters); wide_miss: every that-many-th period the
    estimate misses the start by three bracket widths; nrow_off: every that-many-th period the discovery settled on
    another sample count."""
    ti = 1.0 / f_sf
    ps = freq * 32.0 * ti
    nnat = int(round(f_sf * 1e-3))
    data = np.ones(nnat + 4, np.int8)
    I, Q = np.zeros(nnat + 4, np.int16), np.zeros(nnat + 4, np.int16)
    out, info, same = np.zeros(1), np.zeros(4, np.int32), np.zeros(1, np.int32)
    how = np.zeros(nper, np.int32)
    both = 0
    for e in range(nper):
        n = nnat + (1 if e % 7 == 3 else 0) - (1 if e % 11 == 5 else 0)
        w = max(W0, abs(remcarr) * 2.0 ** -36)
        est = remcarr + float(rng.uniform(-est_err, est_err))
        if wide_miss and e % wide_miss == wide_miss - 1:
            est = remcarr + 3.0 * w
        nrow = n + (1 if nrow_off and e % nrow_off == nrow_off - 1 else 0)
        how[e] = ncr.ncr_period(ps, nnat + 16, remcarr, n, est, w, nrow, out.ctypes.data, info.ctypes.data, same.ctypes.data)
        where = f"freq={freq!r} f_sf={f_sf!r} period {e} remcarr={remcarr!r} n={n} how={how[e]} info={info.tolist()}"
        assert same[0] == 1, f"record's one-binade step against the reference form: {where}"
        both += int(info[3])
        orem = orc.lib().orc_mixcarr_seq(data.ctypes.data, 1, ti, n, freq, remcarr, I.ctypes.data, Q.ctypes.data)
        assert np.float64(orem).view(np.uint64) == out.view(np.uint64)[0], f"chain {out[0]!r} vs oracle {orem!r}: {where}"
        remcarr = float(orem)
    return how, both


def test_falling_channel_across_binades(ncr, orc):
    """-803 rad at -4321.5 Hz: |x| crosses 4096, 8192 and 16384 LUT steps inside the run; the periods that straddle
    a binade leave the record's step, all others take it"""
    how, both = _chain(ncr, orc, -4321.5, 16.368e6, -803.0, np.random.default_rng(7701))
    assert np.sum(how != 2) >= 3, np.bincount(how, minlength=6).tolist()
    assert np.sum(how == 2) >= 0.9 * NPER, np.bincount(how, minlength=6).tolist()
    assert both >= 0.9 * NPER


@pytest.mark.parametrize("freq,f_sf,remcarr", [(-31.0, 16.368e6, -0.5), (-31.0, 4.092e6, -55.0), (-9000.0, 20e6, -1e5),
                                               (-2500.25, 16.368e6, -3.0e6)])
def test_falling_channels(ncr, orc, freq, f_sf, remcarr):
    how, both = _chain(ncr, orc, freq, f_sf, remcarr, np.random.default_rng(7702))
    # (a phase next to zero starts inside the table's window: tag 1 periods, served by the window step)
    assert np.sum((how == 2) | (how == 1)) >= 0.9 * NPER, np.bincount(how, minlength=6).tolist()
    assert np.sum(how == 2) > 0


@pytest.mark.parametrize("freq,f_sf,remcarr", [(8765.25, 16.368e6, 1.0), (200.0, 16.368e6, 0.0), (4321.5, 4.092e6, 6.2),
                                               (4000.0, 4.092e6, 6.2), (-9000.0, 16.368e6, 3.0), (11000.0, 20e6, 1e-7)])
def test_rising_and_grid_channels(ncr, orc, freq, f_sf, remcarr):
    how, _ = _chain(ncr, orc, freq, f_sf, remcarr, np.random.default_rng(7703))
    # (a whole number of turns per period keeps the phase where it started, in time next to zero, where the discovery
    # has no claims: such channels are held to the oracle only)
    if freq > 0 and remcarr > 1e-3 and freq % 1000.0 != 0.0:
        assert np.sum(how == 1) >= 0.9 * NPER, np.bincount(how, minlength=6).tolist()


@pytest.mark.parametrize("freq,remcarr", [(8765.25, 1.0), (-4321.5, -803.0)])
def test_missed_brackets_and_other_sample_counts(ncr, orc, freq, remcarr):
    """a start outside its bracket and a period whose sample count is not the row's never take the window step on
    that row; the chain stays exact"""
    rng = np.random.default_rng(7704)
    how, _ = _chain(ncr, orc, freq, 16.368e6, remcarr, rng, wide_miss=5)
    if freq > 0:
        assert not np.any(how[4::5] == 1), how[4::5].tolist()
    how, _ = _chain(ncr, orc, freq, 16.368e6, remcarr, rng, nrow_off=4)
    if freq > 0:
        assert not np.any(how[3::4] == 1), how[3::4].tolist()
    _chain(ncr, orc, freq, 16.368e6, remcarr, rng, est_err=0.0, nper=60)


def test_one_binade_consts(ncr):
    """d, tie and top from the exponent alone against gc_one_binade_walk: random phases and addends, ties (addend an
    odd multiple of half the grid) from even and odd phases, the top of a binade, both signs"""
    rng = np.random.default_rng(7705)
    bad = 0
    for _ in range(20000):
        s = float(rng.choice([-1.0, 1.0]) * 2.0 ** rng.uniform(-12.0, -3.0))
        x = float(rng.choice([-1.0, 1.0]) * 2.0 ** rng.uniform(-8.0, 40.0))
        bad += 0 if ncr.ncr_consts(x, s, int(rng.integers(1, 70000))) else 1
    for ex in range(8, 30):
        u = 2.0 ** (ex - 52)
        for k in (1, 3, 5, 1001):
            s = -k * u / 2
            for m in (0, 1, 2, 3, 2 ** 51 - 1, 2 ** 52 - 2, 2 ** 52 - 1):
                x = -(2.0 ** ex) - m * u
                for n in (1, 2, 16368):
                    bad += 0 if ncr.ncr_consts(x, s, n) else 1
                    bad += 0 if ncr.ncr_consts(-x, -s, n) else 1
                    bad += 0 if ncr.ncr_consts(x, -s, n) else 1
    assert bad == 0
