"""The code chain as a scan (csrc/gnsscorr_nco.h: gc_code_scan_row, gc_code_scan_next) on the CPU: 300-period chains
taken the way the batch planner's code wavefront takes them -- bracket and claims per period as the discovery finds
them, a scan row from the step at the bracket's ends, the running Y = c0 / u carried from served period to served
period -- against the oracle's literal rescode loop and sdrtracking()'s sample count, bit for bit in remcode, n and
buffloc in every period.

So that the chains cannot pass on fallbacks, at least 90 % of the periods of the random-rate channels are served by
the scan; the exact chip rate from remcode 0 (no brackets) and a chip step that is a tie on the grid u (not scannable)
are served by the step functions and stay exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "nco_scan_host.cpp")
NPER = 300


@pytest.fixture(scope="module")
def ncs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ncs") / "nco_scan_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    d, i, vp = C.c_double, C.c_int, C.c_void_p
    L.ncs_chain.argtypes = [d, i, i, d, d, i, vp, vp, vp, vp, vp]
    return L


def _chain(ncs, orc, crate, f_sf, length, smax, remcode0, rng, est_err=2.0 ** -32):
    """-> (how, info); asserts every period against the oracle"""
    ti = 1.0 / f_sf
    ci = ti * crate                                   # ref src/sdrcmn.c:709
    spc = crate / f_sf                                # ref src/sdrtrk.c:31
    off = rng.uniform(-est_err, est_err, NPER)
    rem, ns, how, info = np.zeros(NPER + 1), np.zeros(NPER, np.int32), np.zeros(NPER, np.int32), np.zeros(3, np.int32)
    rc = ncs.ncs_chain(ci, length, smax, spc, remcode0, NPER, off.ctypes.data, rem.ctypes.data, ns.ctypes.data, how.ctypes.data,
                       info.ctypes.data)
    assert rc == 0
    code = np.arange(length, dtype=np.int16)
    r, buff, mybuff = float(remcode0), 0, 0
    for e in range(NPER):
        where = f"crate={crate!r} f_sf={f_sf!r} len={length} smax={smax} period {e} remcode={r!r} how={how[e]}"
        assert np.float64(r).view(np.uint64) == rem[e:e + 1].view(np.uint64)[0], f"start {rem[e]!r}: {where}"
        n = int((length - r) / spc)                   # ref src/sdrtrk.c:31-32
        assert n == ns[e], f"n {ns[e]}: {where}"
        assert buff == mybuff, where
        out = np.zeros(n + 2 * smax, np.int16)
        r = float(orc.lib().orc_rescode_seq(code.ctypes.data, length, r, smax, ci, n, out.ctypes.data))
        buff += n
        mybuff += int(ns[e])
    assert np.float64(r).view(np.uint64) == rem[NPER:].view(np.uint64)[0]
    assert info[1] == 0, f"carried Y differs from the head's own in {info[1]} periods"
    return how, info


CASES = [(1.023e6, 16.368e6, 1023), (1.023e6, 4.092e6, 1023), (1.023e6, 20e6, 1023), (0.511e6, 16.368e6, 511)]


@pytest.mark.parametrize("crate0,f_sf,length", CASES)
@pytest.mark.parametrize("smax", [3, 6, 18, 30])
def test_random_rate_channels(ncs, orc, crate0, f_sf, length, smax):
    rng = np.random.default_rng(8800 + smax + length)
    for doff in (-12.0, -3.3, 0.41, 7.7, 12.0):
        how, info = _chain(ncs, orc, crate0 + doff, f_sf, length, smax, float(rng.uniform(0.01, 0.99)), rng)
        assert np.sum(how == 1) >= 0.9 * NPER, (doff, np.bincount(how, minlength=3).tolist(), info.tolist())


def test_first_period_on_the_other_side_and_starts_next_to_zero_and_one(ncs, orc):
    rng = np.random.default_rng(8801)
    smax, crate, f_sf = 6, 1.023e6 + 2.5, 16.368e6
    ci = crate / f_sf
    # (remcode >= smax ci: the reference's cs >= 0 branch, which no scan row covers)
    how, _ = _chain(ncs, orc, crate, f_sf, 1023, smax, 0.7, rng)
    assert how[0] == 2 and np.sum(how == 1) >= 0.9 * NPER, how[:4].tolist()
    assert 0.7 - smax * ci >= 0.0
    for r0 in (1e-7, 0.0, 1.0 - 1e-7, 1.0 + 1e-7, 1e-6, 1.0 - 1e-6):
        how, _ = _chain(ncs, orc, crate, f_sf, 1023, smax, r0, rng)
        assert np.sum(how == 1) >= 0.9 * NPER, (r0, np.bincount(how, minlength=3).tolist())


def test_exact_chip_rate_has_no_brackets(ncs, orc):
    """ci = 1/16 from remcode 0: the sums hit their thresholds exactly, nothing is bracketed, every period goes to the
    step functions"""
    how, _ = _chain(ncs, orc, 1.023e6, 16.368e6, 1023, 6, 0.0, np.random.default_rng(8802))
    assert np.all(how == 2)


def test_tie_on_the_top_grid_is_not_scannable(ncs, orc):
    """a chip step that is an odd multiple of u / 2 (u = 2^-43 for 1023 chips; ti = 2^-24 makes ti * crate the chosen
    double exactly): the result depends on the parity of c0 / u, the channel has no scan rows, the chain stays exact"""
    ci = (int(0.0625 * 2.0 ** 44) | 1) * 2.0 ** -44
    crate = ci * 2.0 ** 24
    assert crate * 2.0 ** -24 == ci
    how, info = _chain(ncs, orc, crate, 2.0 ** 24, 1023, 6, 0.3, np.random.default_rng(8803))
    assert info[0] == 0 and np.all(how == 2), (info.tolist(), np.bincount(how, minlength=3).tolist())
