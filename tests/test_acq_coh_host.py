"""Coherent integration (gnsscorr_acq_set_coherent) on the host: that the restatement of its semantics
(tests/acq_coh_cases.py) is the oracle's search for ncoh = 1, that every scenario tests/test_gpu_acq_coherent.py runs
on the device is decided on the restatement with room (every decision acq_cases.MARGIN from a tie, 3*MARGIN from the
threshold, after every group), the sensitivity claim behind the feature on the literal LUT path, and that the library
exports the entry points.  No GPU.

Figures (restatement, 4.092 Msps IQ, PRN 1 at +1000 Hz and lag 1234, sigma 8, intg 10):
  36 dB-Hz, seed 2 (the value the issue starts from; seeds 0, 1 and 3 separate as well, so no step in C/N0 was taken):
    ncoh 1 on +-7 kHz / 200 Hz: peak ratio 1.31 .. 1.85 over the ten iterations, never acquired;
    ncoh 10 on +-5 kHz / 50 Hz: peak ratio 3.98 at lag 1234, bin 120 (+1000 Hz): acquired.
  The same span with the data bit flipped in its middle (sample 5.5 * nsamp): peak ratio 2.85, in bin 121: not
  acquired (ratio to the unflipped span: 0.72).  At 40 dB-Hz (PRN 9, 9 bins) the flipped satellite is still acquired,
  peak ratio 5.95 against 14.2, two bins (100 Hz) off: the flip splits its line to both sides."""
import ctypes as C

import numpy as np
import pytest

import acq_cases as ac
import acq_coh_cases as cc


@pytest.fixture(scope="module")
def scen(gc, orc, synth):
    return lambda name: cc.scenario(gc, orc, synth, name)


@pytest.mark.parametrize("name,chan", [("iq10", (9, 200, 50, 10, 1)), ("real", (13, 1000, 250, 4, 1)),
                                       ("m20", (20, 1000, 250, 4, 1))], ids=["iq", "real", "20M"])
def test_ncoh1_restatement_is_the_oracle(gc, orc, synth, name, chan):
    """ncoh = 1: the restatement against acq_cases.oracle_acq (orc_sdracquisition window by window) -- decisions and
    integers exact, the power array to 1e-9 relative, summed over several windows.  Both dtypes and a 20000-sample
    period."""
    sc = cc.SCEN[name]
    W = cc.make_span(gc, synth, sc)
    n, intg = cc.nsamp(sc), chan[3]
    assert intg == cc.max_intg(sc)
    _, o = cc.pair(gc, orc, sc, chan)
    got = cc.coh_acq(orc, o, W, len(W), len(W), 1)
    want = ac.oracle_acq(orc, o, W, len(W), len(W))
    for k in ("flagacq", "iters", "buffloc", "acqcodei", "freqi", "acqfreq", "b0"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert 1 < want["iters"] <= intg                    # power summed over several windows
    assert len(got["steps"]) == len(want["steps"])
    for a, b in zip(got["steps"], want["steps"]):
        assert a[1:3] == b[1:3] and abs(a[0] - b[0]) <= 1e-9 * abs(b[0])
    for k in ("peakr", "cn0"):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), k
    assert np.all(np.abs(got["P"] - want["P"]) <= 1e-9 * np.abs(want["P"]))
    # the wiped-off integers of a window are the oracle's own, and with them the sum of one term
    zI, zQ, I, Q = cc.group_sum(orc, o, W, len(W), 3 * n, 1, o.freq[1])
    assert np.array_equal(zI, I) and np.array_equal(zQ, Q) and len(zI) == 2 * n


@pytest.mark.parametrize("name", list(cc.SCEN))
def test_every_scenario_is_decided_with_room(scen, name):
    """A condition on the inputs of the device tests: after every group the winning lag and the winning row lead by
    MARGIN, and the peak ratio is 3*MARGIN away from ACQTH."""
    _, pairs, res = scen(name)
    for ch, r in zip(cc.SCEN[name]["chans"], res):
        assert not np.isnan(r["cn0"])
        ac.check_margins(r, (name, ch))
        assert r["groups"] == len(r["steps"]) and r["iters"] == (r["groups"] * ch[4] if r["flagacq"] else ch[3])
        print(name, ch, "acquired" if r["flagacq"] else "not acquired", "iters", r["iters"],
              "peak ratios", [round(s[0], 3) for s in r["steps"]])


def test_scenarios_are_what_the_device_tests_need(scen):
    """iq10: one group of 10; groups of 5 passing at group 1, only at group 2, never.  real / m20 / mixed: acquired at
    the placed lag (+-1) and bin."""
    _, _, (g10, strong, late, absent) = scen("iq10")
    assert (g10["flagacq"], g10["iters"], g10["acqcodei"], g10["freqi"]) == (1, 10, 3210, 5)
    assert (strong["flagacq"], strong["iters"], strong["acqcodei"], strong["freqi"]) == (1, 5, 2345, 5)
    assert (late["flagacq"], late["iters"], late["acqcodei"], late["freqi"]) == (1, 10, 777, 2)
    assert late["steps"][0][0] < 3.0 < late["steps"][1][0]
    assert (absent["flagacq"], absent["iters"]) == (0, 10) and absent["buffloc"] == absent["b0"] + 10 * 4092
    for name in ("real", "m20", "mixed"):
        sc = cc.SCEN[name]
        placed = {s[0]: s for s in sc["sats"]}
        for ch, r in zip(sc["chans"], scen(name)[2]):
            prn, hband, step = ch[:3]
            assert r["flagacq"] and abs(r["acqcodei"] - placed[prn][1]) <= 1, (name, ch)
            assert r["freqi"] == hband // step + round(placed[prn][2] / step), (name, ch)
            assert r["buffloc"] == r["b0"] + r["acqcodei"]
    # the late position of the intg-20 channel's span: b0 of the intg-10 channels lies 10 periods into it
    assert [r["b0"] for r in scen("mixed")[2]] == [10 * 4092] * 3 + [0]


def test_weak_satellite_needs_the_coherent_search(scen):
    """The claim the feature rests on, on the literal LUT path: at 36 dB-Hz the reference's integration (10 x 1 ms on
    +-7 kHz / 200 Hz) acquires at no iteration, one coherent group of 10 ms on +-5 kHz / 50 Hz acquires at the placed
    lag +-1 in the placed bin."""
    sc = cc.SCEN["weak"]
    prn, lag, dop, cn0 = sc["sats"][0][:4]
    assert (prn, cn0, sc["f_sf"]) == (1, 36.0, 4.092e6)
    _, pairs, (r1, r10) = scen("weak")
    assert pairs[0][0].nfreq == 71 and pairs[1][0].nfreq == 201
    assert not r1["flagacq"] and r1["iters"] == 10 and len(r1["steps"]) == 10
    assert all(s[0] < 3.0 for s in r1["steps"])
    assert r10["flagacq"] and r10["iters"] == 10 and len(r10["steps"]) == 1
    assert abs(r10["acqcodei"] - lag) <= 1 and r10["freqi"] == (5000 + int(dop)) // 50
    assert r10["acqfreq"] == dop
    print("weak satellite at %.1f dB-Hz: ncoh 1 peak ratios %s; ncoh 10 peak ratio %.3f at lag %d bin %d, cn0 %.2f"
          % (cn0, [round(s[0], 2) for s in r1["steps"]], r10["peakr"], r10["acqcodei"], r10["freqi"], r10["cn0"]))


def test_bit_flip_in_the_span_loses_the_peak(scen):
    """The same span with the satellite's data bit flipped in its middle: the group of 10 ms no longer passes."""
    r10 = scen("weak")[2][1]
    (rf,) = scen("flip")[2]
    assert r10["flagacq"] and not rf["flagacq"] and rf["peakr"] < 3.0 < r10["peakr"]
    (r40,) = scen("flip40")[2]
    g10 = scen("iq10")[2][0]
    assert r40["flagacq"] and r40["peakr"] < 0.5 * g10["peakr"] and abs(r40["freqi"] - g10["freqi"]) == 2
    print("bit flip in the middle of the span: peak ratio %.3f -> %.3f (x %.2f), bin %d -> %d; at 40 dB-Hz %.2f -> %.2f"
          % (r10["peakr"], rf["peakr"], rf["peakr"] / r10["peakr"], r10["freqi"], rf["freqi"], g10["peakr"], r40["peakr"]))


def test_cn0_uses_the_coherent_time(scen, orc):
    """cn0 of a group result: checkacquisition()'s, over ncoh * ctime."""
    _, pairs, res = scen("iq10")
    for (c, o), r, ch in zip(pairs, res, cc.SCEN["iq10"]["chans"]):
        want = ac._cn0_restated(r["P"], r["acqcodei"], r["freqi"], o.nsampchip, ch[4] * o.ctime)
        assert abs(r["cn0"] - want) <= 1e-9 * abs(want)


def test_library_exports_and_mirror(gc):
    """The .so exports the entry points with the header's limits, and the mirror's sizes are the header's."""
    L = gc.lib()
    for name in ("gnsscorr_acq_set_coherent", "gnsscorr_acq_get_coherent"):
        assert hasattr(L, name) and name in gc.EXPORTS_GNSSCORR
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gnsscorr.h")).read()
    assert "#define GNSSCORR_MAXFREQ   %d " % gc.MAXFREQ in hdr and gc.MAXFREQ == 1024
    assert "#define GNSSCORR_MAXCOH    %d " % gc.MAXCOH in hdr and gc.MAXCOH == 20
    assert L.gnsscorr_acq_set_coherent.argtypes == [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    assert C.sizeof(gc.AcqRes) == 48
    # without a context both refuse (no device needed)
    one = (C.c_int * 1)(1)
    assert L.gnsscorr_acq_set_coherent(None, 0, 1, one) == -1 and L.gnsscorr_acq_get_coherent(None, 0, 1, one) == -1
    # the recommended grid: the reference's step, but at most 1/(2 ncoh ctime)
    assert [gc.coherent_step(k) for k in (1, 2, 5, 10, 20)] == [200, 200, 100, 50, 25]
    c = gc.Channel(1, f_sf=4.092e6, hband=7000, step=gc.coherent_step(10), ncoh=10)
    assert c.nfreq == 281 <= gc.MAXFREQ and c.ncoh == 10 and c.freq[1] - c.freq[0] == 50.0
