"""The closed loop's branch cases (tests/loop_branch_cases.py) on the CPU.

1. Every row of every table reaches the branch it is named for under the oracle alone -- a condition of the device tests
   (tests/test_gpu_loop_branches.py), asserted here from the oracle's state, and no period of a noise row leaves a
   non-finite frequency behind.
2. The oracle's filters (orc_pll / orc_dll) and the product's host twins (pll / dll of sdr_host.c, on an sdrch_t) on
   every filter row, called directly so that a -0.0 sum stays -0.0: equal bit for bit, NaN where NaN; and their distance
   from the mpmath restatement (restate_pll / restate_dll), printed per output field in ulps of the result (DESIGN.md
   section 4 carries the figures) and held to the project's bound of 1e-14 (tests/test_gpu_loop.py::_close)."""
import ctypes as C
import math

import numpy as np
import pytest

import loop_branch_cases as lc

F_SF = 16.368e6
PLL_FIELDS = ("carrErr", "freqErr", "carrNco", "carrfreq")
DLL_FIELDS = ("codeErr", "codeNco", "codefreq")


def _close(a, b, tol=1e-14):
    return abs(a - b) <= tol * max(1.0, abs(a), abs(b))


# ---- filter rows --------------------------------------------------------------------------------------------------
def _restate_row(row, o, prm, dt):
    return lc.restate_row(row, o, prm, dt, through_step=False)


def _oracle_filter_chan(orc, row, taps=(2, 3, 3), dtype=2, f_if=0.0):
    return lc.filter_oracle_chan(orc, row, 3, taps, dtype, f_if)


@pytest.mark.parametrize("row", lc.FILTER_ROWS, ids=[r["name"] for r in lc.FILTER_ROWS])
@pytest.mark.parametrize("dtype,f_if,taps", [(2, 0.0, (6, 3, 6)), (1, 4.092e6, (2, 3, 3))], ids=["iq13", "real5"])
def test_filter_row_reaches_its_branch_through_a_period(orc, row, dtype, f_if, taps):
    """orc_sdrthread_step on a zero ring with the row's sums preset, as the device test runs it: the correlator adds
    exactly 0, the prm1 filters run on the preset sums, and the oracle's outputs show the branch the row is named for."""
    o = _oracle_filter_chan(orc, row, taps, dtype, f_if)
    ntap = 1 + 2 * taps[0]
    assert (o.ne, o.nl) == ((3, 4) if ntap == 13 else (1, 2))
    n = 16368 * 3
    data = lc.make_ring_data("zero", dtype, n)
    ring = orc.make_ring(data, n, n)
    b = C.c_uint64(100)
    p, dll_of = _restate_row(dict(row, sums=_as_step(row["sums"])), o, 0, o.ctime)
    assert orc.lib().orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(b)) == 1
    assert o.flagloopfilter == 1 and o.flagsync == 0 and 16000 < o.currnsamp < 16400
    assert not any(o.II[i] or o.QQ[i] for i in range(ntap))
    assert not any(o.sumI[i] or o.sumQ[i] or o.oldsumI[i] or o.oldsumQ[i] for i in range(ntap))     # cleared
    _assert_branch(row, o, p, dll_of(o.carrfreq), through_step=True)


def _as_step(sums):
    return {k: (v + 0.0) for k, v in sums.items()}          # what cumsumcorr leaves of a preset: -0.0 + 0.0 = +0.0


def _assert_branch(row, o, p, d, through_step):
    br = row["branch"]
    s = _as_step(row["sums"]) if through_step else row["sums"]
    if "ip" in br:
        IP = s["IP"]
        cls = "pos" if IP > 0 else "neg" if IP < 0 else ("-0" if math.copysign(1.0, IP) < 0 else "+0")
        want_cls = "+0" if (through_step and br["ip"] == "-0") else br["ip"]
        assert cls == want_cls, row["name"]
        assert (s["oldIP"] == 0) == bool(br.get("oldip0") or row["name"] == "pll_all_zero"), row["name"]
        # which wrap fired, from the restatement's f1 - f2 -- far enough from +-pi/2 that no rounding decides it
        half = lc.mp.mpf(lc.PI_D) / 2
        assert p["wrap"] == br["wrap"], (row["name"], p["wrap"])
        if "freqErr" not in br:
            assert abs(abs(p["f1mf2"]) - half) > 1e-4, row["name"]
        unwrapped, wrapped_up, wrapped_dn = float(p["f1mf2"]), float(lc.PI_D - p["f1mf2"]), float(-lc.PI_D - p["f1mf2"])
        want = {0: unwrapped, 1: wrapped_up, -1: wrapped_dn}[br["wrap"]]
        assert _close(o.freqErr, want), (row["name"], o.freqErr, want)
        for other in {unwrapped, wrapped_up, wrapped_dn} - {want}:
            assert abs(o.freqErr - other) > 1e-3, (row["name"], o.freqErr, other)
        exact = lc.exact_outputs(row, through_step)
        for f in ("carrErr", "freqErr"):
            if f in exact:
                assert lc.same_double(getattr(o, f), exact[f]), (row["name"], f, getattr(o, f))
    else:
        E, L = math.hypot(s["IE"], s["QE"]), math.hypot(s["IL"], s["QL"])
        kind = "0/0" if E == 0 and L == 0 else "E=0" if E == 0 else "L=0" if L == 0 else "E=L" if E == L else "E>L" if E > L else "E<L"
        assert kind == br["dll"], row["name"]
        if "codeErr" in br:
            assert lc.same_double(o.codeErr, br["codeErr"]), (row["name"], o.codeErr)
        else:
            assert (o.codeErr > 0) == (kind == "E>L") and 0.05 < abs(o.codeErr) < 0.95, (row["name"], o.codeErr)
        assert math.isnan(o.codefreq) == (kind == "0/0") and math.isnan(o.codeNco) == (kind == "0/0"), row["name"]
    # every row: the oracle against the restatement, NaN where NaN
    for f in PLL_FIELDS:
        assert _close(getattr(o, f), float(p[f])), (row["name"], f, getattr(o, f), float(p[f]))
    for f in DLL_FIELDS:
        r = d[f]
        if isinstance(r, float) and math.isnan(r):
            assert math.isnan(getattr(o, f)), (row["name"], f)
        else:
            assert _close(getattr(o, f), float(r)), (row["name"], f, getattr(o, f), float(r))


@pytest.fixture(scope="module")
def host_chan(gc):
    """An sdrch_t of the product's host code with the 5-tap layout (as tests/test_host.py builds it)."""
    L = gc.lib()
    ini = gc.sdrini()
    saved = gc.SdrIni.from_buffer_copy(ini)
    ini.trkcorrn, ini.trkcorrd, ini.trkcorrp = 2, 3, 3
    for i in range(2):                                  # the shipped loop bandwidths (the oracle's defaults)
        ini.trkdllb[i], ini.trkpllb[i], ini.trkfllb[i] = (5.0, 1.0)[i], (30.0, 10.0)[i], (200.0, 50.0)[i]
    sdr = gc.SdrCh()
    assert L.initsdrch(1, gc.SYS_GPS, 9, gc.CTYPE_L1CA, 2, 1, 1575.42e6, F_SF, 0.0, C.byref(sdr)) == 0
    yield sdr
    L.freesdrch(C.byref(sdr))
    C.memmove(C.addressof(ini), C.addressof(saved), C.sizeof(gc.SdrIni))


@pytest.mark.parametrize("prm", [0, 1], ids=["prm1", "prm2"])
def test_filters_oracle_host_twin_and_restatement(gc, orc, host_chan, prm, capsys):
    """orc_pll / orc_dll and the host's pll / dll called directly on every filter row (a -0.0 sum stays -0.0): equal
    bit for bit, the branch of the row reached, and within 1e-14 of the restatement; the ulp distances are printed."""
    L, sdr = gc.lib(), host_chan
    dt = 1e-3 if prm == 0 else 1e-2
    hprm = sdr.trk.prm1 if prm == 0 else sdr.trk.prm2
    lines, worst = [], {}
    for row in lc.FILTER_ROWS:
        o = _oracle_filter_chan(orc, row)
        assert (sdr.trk.ne, sdr.trk.nl) == (o.ne, o.nl) == (1, 2)
        assert (hprm.pllaw, hprm.pllw2, hprm.fllw, hprm.dllaw, hprm.dllw2) == \
            (o.pllaw[prm], o.pllw2[prm], o.fllw[prm], o.dllaw[prm], o.dllw2[prm]) and hprm.pllaw > 0
        sdr.acq.acqfreq = o.acq.acqfreq
        sdr.trk.carrfreq, sdr.trk.codefreq = o.carrfreq, o.codefreq
        for name in ("carrErr", "codeErr", "carrNco", "codeNco"):
            setattr(sdr.trk, name, lc.FILTER_STATE[name])
        for name in ("sumI", "sumQ", "oldsumI", "oldsumQ"):
            for i in range(5):
                getattr(sdr.trk, name)[i] = getattr(o, name)[i]
        assert math.copysign(1.0, o.sumI[0]) == math.copysign(1.0, row["sums"]["IP"])       # (ctypes keeps the zero's sign)
        p, dll_of = _restate_row(row, o, prm, dt)
        orc.lib().orc_pll(C.byref(o), prm, dt)
        orc.lib().orc_dll(C.byref(o), prm, dt)
        L.pll(C.byref(sdr), C.byref(hprm), dt)
        L.dll(C.byref(sdr), C.byref(hprm), dt)
        for f in PLL_FIELDS + DLL_FIELDS:
            assert lc.same_double(getattr(sdr.trk, f), getattr(o, f)), (row["name"], f, getattr(sdr.trk, f), getattr(o, f))
        d = dll_of(o.carrfreq)
        _assert_branch(row, o, p, d, through_step=False)
        u = {f: lc.ulps_from(getattr(o, f), (p if f in p else d)[f]) for f in PLL_FIELDS + DLL_FIELDS}
        lines.append("%-28s " % row["name"] + " ".join("%s %.2f" % (f, u[f]) for f in PLL_FIELDS + DLL_FIELDS))
        for f, x in u.items():
            worst[f] = max(worst.get(f, 0.0), x)
    with capsys.disabled():
        print("\nulps from the restatement, oracle = host twin, prm%d:" % (prm + 1))
        print("\n".join(lines))
        print("worst: " + " ".join("%s %.2f" % kv for kv in worst.items()))
    # (inf: a NaN against a number, or a non-zero value where the restated result is an exact 0)
    assert all(math.isfinite(x) for x in worst.values())


def test_negative_zero_prompt_sum_differs_from_positive_zero(orc):
    """IP = -0.0 with QP = 0 in a direct call: carrErr = atan2(-0.0, +0.0) / PI = -0.0, not the -1 of IP = +0.0 (C Annex
    F.10.1.4); through a period the sum is +0.0 and the two rows coincide."""
    row = next(r for r in lc.FILTER_ROWS if r["name"] == "pll_ip_negzero_qp_zero")
    o = _oracle_filter_chan(orc, row)
    orc.lib().orc_pll(C.byref(o), 0, 1e-3)
    assert lc.same_double(o.carrErr, -0.0)
    p = lc.restate_pll(-0.0, 0.0, 2900.0, 2000.0, 0.0125, 3.75, 1.0, 1.0, 1.0, 1e-3, 0.0)
    assert isinstance(p["carrErr"], float) and lc.same_double(p["carrErr"], -0.0)
    o = _oracle_filter_chan(orc, next(r for r in lc.FILTER_ROWS if r["name"] == "pll_all_zero"))
    orc.lib().orc_pll(C.byref(o), 0, 1e-3)
    assert o.carrErr == -1.0 and o.freqErr == 0.0


# ---- nav and cadence rows -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noise_ring(orc):
    o = orc.make_chan(1, dtype=lc.NAV_FRONT["dtype"], f_sf=lc.NAV_FRONT["f_sf"], f_if=0.0, corrn=1, corrd=2, corrp=2)
    n = o.nsamp * (lc.NAV_NPER + 4)
    data = lc.make_ring_data("noise", lc.NAV_FRONT["dtype"], n, lc.NAV_SEED)
    return data, orc.make_ring(data, n, n)


def _assert_expect(row, x):
    for k, v in row["expect"].items():
        assert x[k] == v, (row["name"], k, x[k], v)
    assert x["finite"], row["name"]                     # no period starts from a non-finite frequency


@pytest.mark.parametrize("row", lc.NAV_ROWS, ids=[r["name"] for r in lc.NAV_ROWS])
def test_nav_row_reaches_its_branch(orc, noise_ring, row):
    x = lc.run_oracle(orc, row, noise_ring[1])
    _assert_expect(row, x)
    pre = row["presets"]
    rate, cnt0 = pre["rate"], pre["cnt"]
    assert 0 < x["sync"] < lc.NAV_CHUNKS[0] + lc.NAV_CHUNKS[1] and x["nbits"] >= 4
    assert x["biti_at_sync"] == (cnt0 + x["sync"]) % rate
    if row["prn"] <= 5:                                 # the vote path: the winning bin, one back, wrapped below 0
        bins = sorted(pre["bitsync"])
        assert cnt0 > 2000 and x["biti_at_sync"] in bins
        assert x["synci"] == (x["biti_at_sync"] - 1) % rate
        assert x["o"].bitsync[x["biti_at_sync"]] == 51
        if "wrap" in row["name"] or bins == [0]:
            assert x["synci"] == rate - 1 and x["at_sync"] == (-rate + 1, 1), row["name"]      # synci < 0 wrapped; diffi == -rate + 1
        if len(bins) == 2:
            assert x["biti_at_sync"] == bins[1] and x["o"].bitsync[bins[0]] == 50, row["name"]
    else:                                               # rate 1: the shortcut once cnt > 2000
        assert rate == 1 and cnt0 + x["sync"] == 2001 and x["at_sync"] == (0, 1)
    if cnt0 >= lc.TWO32 - 1000:                         # the bit phase at the sync is the 64-bit remainder, not the 32-bit one
        c = cnt0 + x["sync"]
        assert c >= lc.TWO32 and (c % lc.TWO32) % rate != x["biti_at_sync"] and x["cnt"] == cnt0 + lc.NAV_NPER


def test_nav_flagpol_negates_the_decided_bits(orc, noise_ring):
    a, b = (lc.run_oracle(orc, next(r for r in lc.NAV_ROWS if r["name"] == n), noise_ring[1]) for n in lc.FLAGPOL_PAIR)
    assert len(a["bits"]) == len(b["bits"]) > 50 and a["bits"] == [-v for v in b["bits"]]
    assert {1, -1} == set(a["bits"])


ALL_CADENCE = lc.CADENCE_ROWS + lc.CNT_ROWS


@pytest.mark.parametrize("row", ALL_CADENCE, ids=[r["name"] for r in ALL_CADENCE])
def test_cadence_row_reaches_its_branch(orc, noise_ring, row):
    x = lc.run_oracle(orc, row, noise_ring[1])
    _assert_expect(row, x)
    pre = row["presets"]
    rate, loopms, cnt0 = pre["rate"], pre["loopms"], pre["cnt"]
    assert x["sync"] == 0 and x["nbits"] in (lc.NAV_NPER // rate, lc.NAV_NPER // rate + 1)
    if loopms > rate:                                   # checkbit()'s counter is reset before it reaches loopms
        assert x["nupd"] <= (1 if pre["navcnt"] == 0 and rate > 1 else 0) and not x["gaps"]      # (navcnt = 0 preset: once)
    elif rate % loopms:                                 # loopms does not divide rate: the gap across the bit edge is longer
        assert loopms + rate % loopms in x["gaps"] and (loopms in x["gaps"] or rate < 2 * loopms)
    elif rate > 1:
        assert loopms in x["gaps"] or x["nupd"] == 1
    if loopms == 20 and rate == 20:
        assert x["gaps"] == {20}                        # a full GC_STEP_KMAX interval
    if cnt0 + lc.NAV_NPER > lc.TWO32:
        hi = cnt0 + lc.NAV_NPER - 1
        assert (hi % lc.TWO32) % rate != hi % rate      # a 32-bit remainder would shift the bit phase
        assert x["cnt"] == cnt0 + lc.NAV_NPER


def test_tables_cover_what_the_issue_lists():
    names = [r["name"] for r in lc.FILTER_ROWS]
    assert len(set(names)) == len(names) == 20
    assert {(r["presets"]["loopms"], r["presets"]["rate"]) for r in lc.CADENCE_ROWS} == \
        {(l, r) for l in (1, 2, 3, 7, 10, 20, 25) for r in (20, 10, 2, 1)}
    assert {r["presets"]["rate"] for r in lc.NAV_ROWS if r["prn"] <= 5} == {20, 10, 2}
    assert {r["presets"]["flagpol"] for r in lc.NAV_ROWS} == {0, 1}
    assert all(r["presets"]["loopms"] <= 100 for r in lc.NAV_ROWS + ALL_CADENCE)      # the oracle divides by 100 / loopms
    assert all(name in [r["name"] for r in lc.CADENCE_ROWS] for name in lc.OBS_ROWS)
    assert np.all(lc.make_ring_data("zero", 2, 8) == 0)
