"""Code-Doppler compensation (gnsscorr_acq_set_codedoppler) on the host: that the restatement of its semantics
(tests/acq_slip_cases.py) is acq_coh_cases.coh_acq / acq_edge_cases.edge_acq bit for bit with f_cf = 0, that every
scenario tests/test_gpu_acq_slip.py runs on the device is decided on the restatement with room (every decision
acq_cases.MARGIN from a tie, 3*MARGIN from the threshold, after every group), the claim behind the feature, the shift
tables' sign, origin and look-back, and that the library exports the entry points.  No GPU.

Figures (restatement; `drift`: 4.092 Msps IQ, PRN 1 at +1000 Hz and lag 1234, sigma 8, intg 40 in 8 groups of 5, 5 bins
500 Hz apart, f_cf 41 MHz: the peak walks 3.5 samples over the groups, 0.5 inside one; shifts of the satellite's bin 0,
0, -1, -1, -2, -2, -3, -3).  The C/N0 was stepped down from 35 dB-Hz by 0.5 dB on seed 2; at 35, 34.5 and 34 both
searches pass; 33.5 dB-Hz is the strongest value at which the uncompensated search fails and the compensated one passes:
  compensated:   peak ratios 1.31 2.05 2.66 2.67 3.05 -- acquired at group 4 (iters 25), lag 1234;
  uncompensated: peak ratios 1.30 2.01 2.35 2.82 2.73 2.55 2.27 2.48 -- never; its best lag is 1230 of its own frame,
                 which starts back = 3 samples later: stream sample 1233, one early.
At 33 dB-Hz neither passes.  Seeds 0, 1 and 3 at 33.5 dB-Hz do not separate by the flag -- the uncompensated search
passes there as well, but later or no earlier, and up to two samples early (lags in the compensated frame):
  seed 0: compensated group 4 (3.55) at lag 1234, uncompensated group 5 (3.09) at lag 1232;
  seed 1: compensated group 6 (3.65) at lag 1234, uncompensated group 7 (3.12) at lag 1232;
  seed 3: both at group 1 (3.21 / 3.16), lags 1234 / 1234.
The walk is under a chip (4 samples) and the correlation triangle two chips wide: the smear costs about half a dB here."""
import ctypes as C

import numpy as np
import pytest

import acq_cases as ac
import acq_coh_cases as cc
import acq_edge_cases as ec
import acq_slip_cases as sl


@pytest.fixture(scope="module")
def scen(gc, orc, synth):
    return lambda name: sl.scenario(gc, orc, synth, name)


def _same(a, b, keys):
    for k in keys:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k
        elif isinstance(a[k], list) and a[k] and isinstance(a[k][0], np.ndarray):
            assert [x.tobytes() for x in a[k]] == [x.tobytes() for x in b[k]], k
        else:
            assert repr(a[k]) == repr(b[k]), (k, a[k], b[k])        # (repr: NaN equals NaN)


def test_without_a_carrier_the_restatement_is_coh_acq_bit_for_bit(gc, orc, synth):
    """f_cf = 0: slip_acq is coh_acq, and with hypotheses edge_acq, in every returned field and power byte; groups of 5
    passing late and never, and one group of 10 with a flipped bit."""
    sc = cc.SCEN["iq10"]
    W = cc.make_span(gc, synth, sc)
    for chan in sc["chans"][1:]:
        _, o = cc.pair(gc, orc, sc, chan)
        want = cc.coh_acq(orc, o, W, len(W), len(W), chan[4])
        got = sl.slip_acq(orc, o, W, len(W), len(W), chan[4], 0.0)
        _same(got, want, want.keys())
        assert got["back"] == 0 and not got["shifts"].any()
    sc = ec.SCEN["groups5"]
    W = ec.make_span(gc, synth, sc)
    for chan in sc["chans"][:2]:
        _, o = ec.pair(gc, orc, sc, chan)
        want = ec.edge_acq(orc, o, W, len(W), len(W), chan[4], chan[5])
        got = sl.slip_acq(orc, o, W, len(W), len(W), chan[4], 0.0, chan[5])
        _same(got, want, want.keys())
    # the time-domain power as well
    lags = np.array([0, 5, 777, 4091])
    _, o = cc.pair(gc, orc, cc.SCEN["iq10"], cc.SCEN["iq10"]["chans"][2])
    W = cc.make_span(gc, synth, cc.SCEN["iq10"])
    a = cc.coh_power_td(orc, o, W, len(W), 0, 2, 5, lags)
    b = sl.slip_power_td(orc, o, W, len(W), 0, 2, 5, np.zeros((o.nfreq, 2), np.int32), lags)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(sl.SCEN))
def test_every_scenario_is_decided_with_room(scen, name):
    """A condition on the inputs of the device tests: after every group the winning lag and the winning row lead by
    MARGIN and the peak ratio is 3*MARGIN away from ACQTH (with hypotheses: acq_edge_cases.check_margins' conditions)."""
    _, pairs, res = scen(name)
    for ch, r in zip(sl.SCEN[name]["chans"], res):
        assert not np.isnan(r["cn0"])
        if ch[5]:
            ec.check_margins(r, (name, ch))
        else:
            ac.check_margins(r, (name, ch))
        assert r["groups"] == len(r["steps"]) and r["iters"] == (r["groups"] * ch[4] if r["flagacq"] else ch[3])
        print(name, ch, "acquired" if r["flagacq"] else "not acquired", "iters", r["iters"], "lag", r["acqcodei"], "bin",
              r["freqi"], "back", r["back"], "peak ratios", [round(s[0], 3) for s in r["steps"]])


def test_drift_separates_the_two_searches(scen):
    """The claim the feature rests on: at DRIFT_CN0 the search without compensation passes at no group and the
    compensated one passes, at the placed lag (the lag of group 0's frame) in the placed bin."""
    sc = sl.SCEN["drift"]
    prn, lag, dop, cn0 = sc["sats"][0][:4]
    assert (cn0, sc["chans"][0][6], sc["chans"][1][6]) == (sl.DRIFT_CN0, sl.F41, 0.0)
    _, pairs, (comp, plain) = scen("drift")
    assert comp["flagacq"] and comp["acqcodei"] == lag and comp["freqi"] == 4 and comp["acqfreq"] == dop
    assert comp["groups"] >= 4                          # late enough for the walk to matter
    assert not plain["flagacq"] and len(plain["steps"]) == 8 and all(s[0] < 3.0 for s in plain["steps"])
    assert comp["buffloc"] == comp["b0"] + lag and comp["b0"] == 0 and plain["b0"] == comp["back"] == 3
    # the satellite's bin walks half a sample per group
    assert comp["shifts"][4].tolist() == [0, 0, -1, -1, -2, -2, -3, -3]
    print("drift at %.1f dB-Hz: compensated %s; uncompensated %s (lag %d)"
          % (cn0, [round(s[0], 2) for s in comp["steps"]], [round(s[0], 2) for s in plain["steps"]], plain["acqcodei"]))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_drift_on_other_noise(gc, orc, synth, seed):
    """Seeds 0..3 at DRIFT_CN0: the compensated search acquires within a sample of the placed lag and no later than the
    uncompensated one, whose best lag is the placed one or up to the walk of 3.5 samples early."""
    sc = sl.SCEN["drift"]
    pairs = [sl.pair(gc, orc, sc, ch) for ch in sc["chans"]]
    W = sl.make_span(gc, synth, sc, pairs, seed=seed)
    comp, plain = sl.restate(orc, pairs, sc["chans"], W, len(W), len(W))
    lag = sc["sats"][0][1]
    assert comp["flagacq"] and abs(comp["acqcodei"] - lag) <= 1 and comp["freqi"] == 4
    assert comp["iters"] <= plain["iters"]
    assert lag - 4 <= plain["acqcodei"] + plain["b0"] - comp["b0"] <= lag
    print("seed", seed, "compensated", comp["flagacq"], comp["iters"], comp["acqcodei"], [round(s[0], 2) for s in comp["steps"]],
          "uncompensated", plain["flagacq"], plain["iters"], plain["acqcodei"], [round(s[0], 2) for s in plain["steps"]])


def test_shift_tables(scen):
    """Every scenario's tables: s(b, 0) = 0, a positive Doppler starts later groups earlier (s <= 0, falling with g), a
    negative one later, the centre bin not at all; back = max(0, max s); b0 = wrpos - back - (intg + 1) n."""
    for name, sc in sl.SCEN.items():
        W, pairs, res = scen(name)
        for ch, (c, o), r in zip(sc["chans"], pairs, res):
            s, back = r["shifts"], r["back"]
            G, mid = ch[3] // ch[4], (o.nfreq - 1) // 2
            assert s.shape == (o.nfreq, G) and not s[:, 0].any() and not s[mid].any()
            assert back == max(0, int(s.max())) and r["b0"] == len(W) - back - (ch[3] + 1) * o.nsamp and r["b0"] >= 0
            if ch[6] == 0:
                assert not s.any() and back == 0
                continue
            assert np.all(s[mid + 1:] <= 0) and np.all(np.diff(s[mid + 1:], axis=1) <= 0) and s[-1, -1] < 0
            assert np.all(s[:mid] >= 0) and np.all(np.diff(s[:mid], axis=1) >= 0) and s[0, -1] == back > 0
            assert np.array_equal(s[:mid], -s[:mid:-1])             # a symmetric grid: the table is odd in the bin
            assert np.abs(s).max() <= o.nsamp
    assert scen("l1")[2][0]["shifts"].tolist() == [[0, 0, 1, 1, 1, 1, 2, 2, 2, 2], [0] * 10, [0, 0, -1, -1, -1, -1, -2, -2, -2, -2]]
    assert scen("m20")[2][0]["back"] == 12
    # a carrier so large that nothing moves: the table the device test runs the compensating kernel with
    s, back = sl.shifts(np.array([-7000.0, 0.0, 7000.0]), 0.0, 0.0, 1e30, 10, 20, 16368)
    assert not s.any() and back == 0


def test_scenarios_are_what_the_device_tests_need(scen):
    """neg: back > 0 with the satellite in the lowest bin; l1: both satellites pass after the shifts have reached +-1,
    the absent PRN runs all ten groups; edge: passes after the group with the flipped bit, which chose h = 2; m20: the
    second group; mixed: every channel acquired at the placed lag of its own frame, +-1 where compensated with the right
    carrier."""
    (sat, absent) = scen("neg")[2]
    assert sat["flagacq"] and sat["freqi"] == 0 and sat["acqcodei"] == 2345 and sat["back"] == 3 and sat["groups"] >= 3
    assert not absent["flagacq"] and absent["buffloc"] == absent["b0"] + 40 * 4092
    a, b, absent = scen("l1")[2]
    assert (a["flagacq"], a["freqi"], b["flagacq"], b["freqi"]) == (1, 2, 1, 0) and a["groups"] >= 3 and b["groups"] >= 3
    assert abs(a["acqcodei"] - 3210) <= 1 and abs(b["acqcodei"] - 3000) <= 1
    assert not absent["flagacq"] and len(absent["steps"]) == 10
    (e,) = scen("edge")[2]
    assert e["flagacq"] and e["groups"] > 2 and e["hsel"][1][4] == 2 and abs(e["acqcodei"] - 1234) <= 1
    (m,) = scen("m20")[2]
    assert m["flagacq"] and m["groups"] == 2 and abs(m["acqcodei"] - 12345) <= 1 and m["freqi"] == 5
    res = scen("mixed")[2]
    assert all(r["flagacq"] for r in res) and [r["back"] for r in res] == [3, 2, 0, 0, 3]
    assert abs(res[0]["acqcodei"] - 100) <= 1 and abs(res[4]["acqcodei"] - 1500) <= 1 and res[3]["acqcodei"] == 3210 - 3
    assert 1500 - 3 - 4 <= res[2]["acqcodei"] <= 1500 - 3       # uncompensated: its frame starts 3 later; up to the walk early


def test_library_exports_and_mirror(gc):
    """The .so exports the three entry points, the mirror binds them, and without a context they refuse."""
    L = gc.lib()
    for name in ("gnsscorr_acq_set_codedoppler", "gnsscorr_acq_get_codedoppler", "gnsscorr_acq_fetch_shifts"):
        assert hasattr(L, name) and name in gc.EXPORTS_GNSSCORR
    assert L.gnsscorr_acq_set_codedoppler.argtypes == [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
    one = (C.c_double * 1)(1575.42e6)
    assert L.gnsscorr_acq_set_codedoppler(None, 0, 1, one) == -1 and L.gnsscorr_acq_get_codedoppler(None, 0, 1, one) == -1
    back = C.c_int(0)
    assert L.gnsscorr_acq_fetch_shifts(None, 0, None, C.byref(back)) == -1
    c = gc.Channel(3, f_sf=4.092e6, cdop=True)
    assert c.cdop and c.f_cf == 1575.42e6 and not gc.Channel(3).cdop
    g = gc.Channel(-3, ctype=gc.CTYPE_G1, f_sf=4.092e6, cdop=True) if hasattr(gc, "CTYPE_G1") else None
    assert g is None or g.f_cf == 1.60200e9 + 0.56250e6 * -3
