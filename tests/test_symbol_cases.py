"""CPU checks of tests/symbol_cases.py: every scenario tests/test_gpu_symbols_receiver.py asserts exactly is decided
by the oracle with room -- each search acquires, or fails, with its peak ratio 1e-3 relative away from ACQTH and from a
tie, and each channel that follows a satellite keeps the prompt power the existing closed-loop test asks for.  The
margins are printed (-s)."""
import ctypes as C

import numpy as np
import pytest

import acq_cases as ac
import symbol_cases as sc
from test_nco_host import nco          # noqa: F401  (the NCO header on the host)


@pytest.fixture(scope="module")
def rec(gc, synth):
    return sc.recordings(gc, synth)


def _ring(orc, rec, c, wrpos):
    buf = rec[c["ring"] - 1]
    return orc.make_ring(buf, len(buf), wrpos)


def _acq_margins(orc, rec, c, wrpos, where):
    """Window by window (every decision on the way keeps its margin) and as one search (what the GPU test compares)."""
    w = ac.oracle_acq(orc, ac.grid(sc.oracle_chan(orc, c), 7000, 200, 10), rec[c["ring"] - 1], len(rec[c["ring"] - 1]), wrpos)
    ac.check_margins(w, where)
    full = sc.oracle_acq_full(orc, sc.oracle_chan(orc, c), _ring(orc, rec, c, wrpos))
    assert (full["flagacq"], full["iters"], full["buffloc"], full["peakr"]) == (w["flagacq"], w["iters"], w["buffloc"], w["peakr"])
    gaps = min(min(g[3], g[4]) for g in w["steps"])
    print(f"\n{where}: flagacq {w['flagacq']} at iteration {w['iters']}, peakr {w['peakr']:.3f} "
          f"(|peakr - ACQTH| / ACQTH = {abs(w['peakr'] - 3) / 3:.3g}), smallest lag/row gap {gaps:.3g}")
    return w


def test_reinit_searches_acquire_with_margin(orc, rec):
    """Case 3(b), 3(c): PRN A, then PRN B at the same address; PRN C on the other front end."""
    wrpos = sc.ACQ_NBLOCKS * sc.BLK
    found = {}
    for prn, ring in ((sc.ACQ_A, 1), (sc.ACQ_B, 1), (sc.ACQ_C, 2)):
        w = _acq_margins(orc, rec, sc.chan("acq", ring, "A", prn), wrpos, f"re-init PRN {prn} ring {ring}")
        assert w["flagacq"] == 1
        found[prn] = (w["acqcodei"], w["freqi"])
    # the demonstration needs the two satellites apart: the old engine's answer is not the new channel's
    assert found[sc.ACQ_A] != found[sc.ACQ_B]


@pytest.mark.parametrize("lap", sc.WRAP_LAPS)
def test_wrap_searches_with_margin(orc, rec, lap):
    """Case 4: the write position two blocks past the ring's end; the strong satellite at the first window, the weak one
    at a window that straddles the end, the absent one never."""
    fb0, _ = sc.wrap_segment(lap)
    wrpos = (fb0 + sc.NB_WRAP) * sc.BLK
    end = (fb0 + sc.WRAP_BEFORE) * sc.BLK                      # file position of the ring's end
    b0 = wrpos - 11 * sc.NSAMP
    res = [_acq_margins(orc, rec, sc.chan("w", 1, "A", p), wrpos, f"wrap lap {lap} PRN {p}") for p in sc.WRAP_ACQ]
    assert res[0]["flagacq"] == 1 and res[0]["iters"] == 1
    assert res[2]["flagacq"] == 0 and res[2]["iters"] == 10
    straddling = [k + 1 for k in range(10) if b0 + k * sc.NSAMP < end < b0 + (k + 2) * sc.NSAMP]
    assert straddling and res[1]["flagacq"] == 1 and res[1]["iters"] >= straddling[0], (res[1]["iters"], straddling)


def _tracked(orc, rec, chans, fpos0, nper, wrpos, salt=0):
    out = {}
    for c in chans:
        o = sc.oracle_chan(orc, c)
        acqfreq, b = sc.start_state(c, fpos0, salt)
        sc.hand_over(o, acqfreq, o.crate)
        rows, b1 = sc.oracle_track(orc, o, _ring(orc, rec, c, wrpos), b, nper)
        assert b1 < wrpos - sc.NSAMP
        out[c["key"]] = rows
        if sc.sat_of(c) is not None:
            ip = sc.prompt_power(rows)
            print(f"\n{c['key']} from {fpos0}: min prompt power {min(ip):.3g} = {min(ip) / sc.POWER_FLOOR:.1f} x the floor")
            assert min(ip) > sc.POWER_FLOOR, (c["key"], min(ip))
    return out


def test_mixed_receiver_groups_and_power(orc, rec):
    """Case 1: the batch must split into several groups of several members, taps A and B share a group and differ in
    smax, and the channels on a satellite hold it."""
    groups = {}
    for c in sc.MIXED:
        groups.setdefault((sc.ringcfg(c)["dtype"], sc.TAPS[c["taps"]][0]), []).append(c)
    assert len(groups) == 4 and all(len(g) >= 2 for g in groups.values())
    assert {c["ctype"] for c in groups[(2, 2)]} == {sc.CTYPE_L1CA, sc.CTYPE_G1}
    for (_, corrn), g in groups.items():
        if corrn == 2:
            assert {sc.TAPS[c["taps"]][0] * sc.TAPS[c["taps"]][1] for c in g} == {6, 16}          # two smax in one group
    assert len(sc.MIXED) <= 32
    assert sum(sc.sat_of(c) is not None for c in sc.MIXED) == 6
    _tracked(orc, rec, sc.MIXED, 0, sc.MIXED_NPER, sc.NB_LOW * sc.BLK)


def test_reinit_and_wrap_tracking_power(orc, rec):
    """Cases 3(a) and 4: every stretch tracked there starts on its satellite."""
    _tracked(orc, rec, sc.REINIT, 0, sc.REINIT_NPER, sc.NB_LOW * sc.BLK)
    for lap in sc.WRAP_LAPS:
        fb0, _ = sc.wrap_segment(lap)
        end = (fb0 + sc.WRAP_BEFORE) * sc.BLK
        rows = _tracked(orc, rec, sc.WRAP_TRK, end - sc.WRAP_TRK_BACK, sc.WRAP_NPER, (fb0 + sc.NB_WRAP) * sc.BLK, salt=lap)
        for c in sc.WRAP_TRK:
            # periods start before the ring's end and finish after it
            _, b = sc.start_state(c, end - sc.WRAP_TRK_BACK, lap)
            starts = np.cumsum([b] + [r[0][0] for r in rows[c["key"]]])
            assert starts[0] < end < starts[-1] and any(s < end < s + sc.NSAMP - 200 for s in starts[:-1])


def test_edge_states_tell_the_two_smax_apart(nco):          # noqa: F811
    """Every EDGE_STATES entry: the replica walk from coff - 6 ci and the one from coff - 16 ci (what a member of smax 6
    would get if it were handed its group's largest smax) choose different chips at a position all five taps read."""
    def chips(coff, smax, ci, n=64):
        out, rem = np.zeros(n + 2 * smax, np.int32), C.c_double()
        assert nco.nco_code(1023, coff, smax, ci, n, 256, out.ctypes.data, C.byref(rem)) > 0
        return out
    own, other = sc.TAPS["A"][0] * sc.TAPS["A"][1], sc.TAPS["B"][0] * sc.TAPS["B"][1]
    assert (own, other) == (6, 16) and len(sc.EDGE_STATES) == 24
    for coff, dc in sc.EDGE_STATES:
        ci = (1 / sc.F_SF) * (1.023e6 + dc)
        a, b = chips(coff, own, ci), chips(coff, other, ci)
        diff = np.flatnonzero(a != b[other - own:other - own + len(a)])
        assert diff.size and own <= diff[0] < own + 64, (coff, dc, diff)
    groups = {(sc.ringcfg(c)["dtype"], sc.TAPS[c["taps"]][0]) for c in sc.EDGE}
    assert len(groups) == 1 and {c["taps"] for c in sc.EDGE} == {"A", "B"}


def test_many_structs_exceed_the_table():
    assert sc.MANY_FIRST <= 256 < sc.MANY_FIRST + sc.MANY_BATCH - sc.MANY_KNOWN[0]
    assert sc.MANY_FIRST + sum(sc.MANY_BATCH - k for k in sc.MANY_KNOWN) == 264
    assert sc.MANY_BATCH <= 32


def test_oracle_maxvd_is_the_reference_loop(orc):
    """orc_maxvd as the tests of maxvd() lean on it: element 0 seeds the maximum, a NaN there stays (index 0), a NaN
    elsewhere never wins, the first of equal maxima wins (ref src/sdrcmn.c:461-476)."""
    O = orc.lib()
    i = C.c_int()
    d = np.array([np.nan, 5.0, 7.0, 1.0])
    assert np.isnan(O.orc_maxvd(d.ctypes.data, 4, -1, -1, C.byref(i))) and i.value == 0
    d = np.array([2.0, np.nan, 7.0, 7.0, np.nan])
    assert O.orc_maxvd(d.ctypes.data, 5, -1, -1, C.byref(i)) == 7.0 and i.value == 2
    assert O.orc_maxvd(d.ctypes.data, 5, 2, 3, C.byref(i)) == 2.0 and i.value == 0
    d = np.array([1.0, 9.0, 3.0])
    assert O.orc_maxvd(d.ctypes.data, 3, 2, 0, C.byref(i)) == 9.0 and i.value == 1        # wrapped window: 2, 0 excluded
    assert O.orc_maxvd(d.ctypes.data, 3, 1, 0, C.byref(i)) == 1.0 and i.value == 0        # everything but the seed
