"""The value-only period steps (csrc/gnsscorr_nco.h: gc_carrier_value_step, gc_carrier_value_step_one,
gc_code_value_step) against the claims steps they stand in for on the planner chains' bracketed path, and against
the oracle's literal mixcarr / rescode loops, on the CPU.

Bar: for every start whose claims the discovery finds, the value step returns the same double as the claims step
(bit for bit) and as the reference's sequential loop.  The sweeps cover every window position the carrier's
period can start at, every count of subtractions of DPI the claims allow, falling phases (one-binade periods),
the tie binade, every count of literal additions that occurs and every tail length of each tail class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "nco_value_host.cpp")
DPI = 2.0 * 3.1415926535897932
CWIN, PREM = 11, 12
TAILS = (8, 15, 32)


@pytest.fixture(scope="module")
def nvs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("nvs") / "nco_value_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    d, i, vp = C.c_double, C.c_int, C.c_void_p
    L.nvs_carrier.argtypes = [d, i, d, i, vp, vp, vp]
    L.nvs_code.argtypes = [d, i, i, d, i, i, vp, vp, vp]
    return L


def _carrier(nvs, orc, freq, ti, remcarr, n, seen):
    ps = freq * 32.0 * ti
    val, ok, info = np.zeros(3), np.zeros(3, np.int32), np.zeros(5, np.int32)
    tag = nvs.nvs_carrier(ps, int(round(1e-3 / ti)) + 16, remcarr, n, val.ctypes.data, ok.ctypes.data, info.ctypes.data)
    if tag == 0:
        return 0
    where = f"freq={freq!r} ti={ti!r} remcarr={remcarr!r} n={n} info={info.tolist()}"
    assert ok[0] and ok[1] and ok[2], f"claims discovered at this start do not hold: {where} ok={ok.tolist()}"
    data = np.ones(n, np.int8)
    I, Q = np.zeros(n, np.int16), np.zeros(n, np.int16)
    orem = orc.lib().orc_mixcarr_seq(data.ctypes.data, 1, ti, n, freq, remcarr, I.ctypes.data, Q.ctypes.data)
    v = val.view(np.uint64)
    assert v[2] == v[0] and v[2] == v[1], f"value step {val[2]!r} vs claims steps {val[0]!r} / {val[1]!r}: {where}"
    assert val[2] == orem and np.float64(orem).view(np.uint64) == v[2], f"value step {val[2]!r} vs oracle {orem!r}: {where}"
    p0, nseg, kprem, ptie = (int(x) for x in info[1:])
    if tag == 1:
        seen["p0"].add(p0)
        seen["kprem"].add(kprem)
        if ptie >= 0 and p0 <= ptie <= p0 + nseg - 1:
            seen["tie"] += 1
    else:
        seen["one"] += 1
        seen["kprem_one"].add(kprem)
    return tag


def _starts(rng, k):
    """period starts (remcarr) over every binade of (0, 2 pi], next to zero and at 2 pi"""
    lg = DPI * 2.0 ** -rng.uniform(0.0, 14.0, k)
    return list(lg) + [1e-7, 3.3e-7, 1e-6, DPI, np.nextafter(DPI, 0.0), DPI / 2]


def _seen():
    return dict(p0=set(), kprem=set(), kprem_one=set(), tie=0, one=0)


def test_carrier_value_step_window_and_remainder(nvs, orc):
    rng = np.random.default_rng(4401)
    seen = _seen()
    for f_sf in (16.368e6, 4.092e6, 20e6):
        ti = 1 / f_sf
        n = int(f_sf * 1e-3)
        freqs = [200.0 * k for k in range(1, 61)] + list(rng.uniform(50.0, 12000.0, 16))
        for freq in freqs:
            for remcarr in _starts(rng, 12):
                for dn in (0, -1, 1):
                    _carrier(nvs, orc, float(freq), ti, float(remcarr), n + dn, seen)
    # (a period that starts in the window's top binade stays in it: the discovery files it as one binade, tag 2)
    assert seen["p0"] >= set(range(CWIN - 1)), f"window positions reached: {sorted(seen['p0'])}"
    assert seen["kprem"] >= set(range(PREM + 1)), f"counts of subtractions reached: {sorted(seen['kprem'])}"


def test_carrier_value_step_tie_binade(nvs, orc):
    """addends that lie exactly half way between two grid points of a window binade (ti = 2^-24: the reference's
    ps = freq * 32 * ti is the chosen double exactly)"""
    rng = np.random.default_rng(4402)
    seen = _seen()
    ti = 2.0 ** -24
    n = 16777
    for sh in (44, 46, 48, 50, 52):
        for target in (0.0021, 0.0049, 0.0098, 0.0131, 0.0205):
            ps = (int(target * 2.0 ** sh) | 1) * 2.0 ** -sh
            freq = ps * 2.0 ** 19
            assert freq * 32.0 * ti == ps
            for remcarr in _starts(rng, 16):
                _carrier(nvs, orc, freq, ti, float(remcarr), n, seen)
    assert seen["tie"] > 50, f"periods through the tie binade: {seen['tie']}"


def test_carrier_value_step_falling_and_one_binade(nvs, orc):
    rng = np.random.default_rng(4403)
    seen = _seen()
    ti = 1 / 16.368e6
    for freq in list(-rng.uniform(50.0, 10000.0, 24)) + [-200.0 * k for k in range(1, 51)] + [0.5, 3.0, 20.0]:
        for remcarr in list(-10.0 ** rng.uniform(2.0, 6.0, 8)) + list(_starts(rng, 4)):
            _carrier(nvs, orc, float(freq), ti, float(remcarr), 16368, seen)
    assert seen["one"] > 500, f"one-binade periods: {seen['one']}"
    assert 0 in seen["kprem_one"]


def test_code_value_step(nvs, orc):
    rng = np.random.default_rng(4404)
    length = 1023
    code = np.arange(length, dtype=np.int16)
    seen = {t: set() for t in TAILS}
    nl_seen, i0_seen, tie = set(), set(), 0
    cases = []
    for f_sf in (16.368e6, 4.092e6, 20e6, 2.0 ** 24, 65.472e6):
        for _ in range(5):
            cases.append((1.023e6 + float(rng.uniform(-12.0, 12.0)), 1 / f_sf))
    ti = 2.0 ** -24
    for sh in (45, 47, 49):                         # ties in binades below the top one
        ci = (int(0.0625 * 2.0 ** sh) + 1 | 1) * 2.0 ** -sh
        cases.append((ci * 2.0 ** 24, ti))
    for codefreq, ti in cases:
        ci = ti * codefreq
        for smax in (1, 2, 4, 6, 8, 15):
            # a tracked channel's period starts at remcode in [-smax ci, smax ci) (what the step before returns)
            sci = smax * ci
            for remcode in list(rng.uniform(-sci, sci, 4)) + [-sci * (1 - 1e-9), -1e-7, 0.0, 1e-7]:
                nat = int((length - remcode) / ci)
                for dn in range(-4, 20):
                    n = nat + dn
                    nt = n + 2 * smax
                    rc = np.zeros(nt, np.int16)
                    orem = None
                    for tmax in TAILS:
                        val, ok, info = np.zeros(3), np.zeros(3, np.int32), np.zeros(6, np.int32)
                        if not nvs.nvs_code(ci, length, smax, float(remcode), nt, tmax, val.ctypes.data, ok.ctypes.data,
                                            info.ctypes.data):
                            continue
                        where = f"ci={ci!r} smax={smax} remcode={remcode!r} n={n} tmax={tmax} info={info.tolist()}"
                        assert ok[0] and ok[1], f"claims discovered at this start do not hold: {where}"
                        if orem is None:
                            orem = orc.lib().orc_rescode_seq(code.ctypes.data, length, float(remcode), smax, ci, n,
                                                             rc.ctypes.data)
                        v = val.view(np.uint64)
                        assert v[2] == v[0] and v[2] == v[1], f"value step {val[2]!r} vs claims {val[0]!r} / {val[1]!r}: {where}"
                        assert np.float64(orem).view(np.uint64) == v[2], f"value step {val[2]!r} vs oracle {orem!r}: {where}"
                        seen[tmax].add(int(info[4]))
                        nl_seen.add(int(info[2]))
                        i0_seen.add(int(info[3]))
                        tie += 1 if info[5] >= 0 else 0
    for tmax in TAILS:
        assert seen[tmax] >= set(range(1, tmax + 1)), f"tail lengths of class {tmax}: {sorted(seen[tmax])}"
    # (after the wrap y < ci and the table starts at b0 = 4 * 2^exponent(ci), in (2 ci, 4 ci]: two to four additions)
    assert nl_seen == {2, 3, 4}, f"literal additions: {sorted(nl_seen)}"
    assert 0 in i0_seen and i0_seen <= {0, 1}
    assert tie > 0
