"""Reconfiguration of a live context, the part that needs no GPU (the device part is
tests/test_gpu_reconfig.py, the shared inputs tests/reconfig_cases.py).

1. Every search the device tests hold against the oracle is decided with the margin acq_cases.MARGIN, on the oracle and
   the restatements alone: the scenarios iq4 (with the extra absent PRN), real4, coh with its settings and as the plain
   search a channel set is after gnsscorr_set_channels, m26 with its second channel, and the receiver schedule's
   searches of the hand-over signal at every write position its steps end at.  The present satellites are acquired, the
   absent PRNs are not.
2. The refusals.  gnsscorr_create needs a device, so no context exists here and every refusal that depends on a
   context's state -- gnsscorr_ring_create under live channels, GNSSCORR_ESTATE of the schedule's calls after a
   reconfiguration, gnsscorr_acq_set_bitedge on the 65536-point transform, gnsscorr_spec_fetch after
   gnsscorr_set_channels, a search before the ring is refilled -- stays in tests/test_gpu_reconfig.py.  What runs here is
   the argument check in front of them: each reconfiguring entry point refuses a null context with its documented
   code and a message, without touching a device.
3. The comparison helpers themselves: freeze / diff tell apart what np.array_equal cannot (NaN payloads, signed zeros)
   and name the element."""
import ctypes as C
import os

import numpy as np
import pytest

import acq_edge_cases as ec
import acq_fine_cases as fc
import reconfig_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -1, -3


@pytest.mark.parametrize("name,plain", [(n, False) for n in rc.SEARCHED] + [("coh", True)])
def test_scenario_searches_are_decided_with_margin(gc, orc, synth, name, plain):
    want = rc.wants(gc, orc, synth, name, plain)
    assert sorted(want) == sorted(s[0] for s in rc.scen_specs(name))
    for prn, w in want.items():
        rc.check_margins(w, (name, plain, prn))
        assert bool(w["flagacq"]) == (prn in rc.present(name)), (name, plain, prn)
        print(f"{name}{' plain' if plain else ''} prn {prn}: acquired {w['flagacq']} iters {w['iters']} peakr {w['peakr']:.3f} "
              f"edge {w['edge']}")
    if name == "coh":
        # the settings matter: with them the edge is found, without them the search is the reference's
        assert (want[9]["edge"] > 0) == (not plain) and want[9]["ncoh"] == (1 if plain else 10)
    assert any(w["flagacq"] for w in want.values()) and (name in ("coh", "real4") or not all(w["flagacq"] for w in want.values()))


def test_schedule_searches_are_decided_with_margin(gc, orc, synth):
    want = rc.rx_wants(gc, orc, synth)
    assert sorted(want) == rc.RX_WRPOS and rc.RX_WRPOS[-1] <= rc.RX_RING and set(rc.RX_B) == set(rc.RX_A)
    for wp, per in want.items():
        for prn, w in per.items():
            rc.check_margins(w, ("rx", wp, prn))
            assert bool(w["flagacq"]) == (prn in fc.HO_PRNS[:2]), (wp, prn)
            # an acquired channel starts tracking inside what the ring holds at that step
            assert not w["flagacq"] or wp - 11 * rc.N4 <= w["buffloc"] < wp - 10 * rc.N4
    # the pause is shorter than a step, so a failed search is due again at every step
    assert int(rc.RX_RETRY_MS * 1e-3 * rc.F4) < rc.RX_STEP * rc.N4
    assert all(b - a == rc.RX_STEP * rc.N4 for a, b in zip(rc.RX_WRPOS, rc.RX_WRPOS[1:]))


def test_channel_sets_fit_the_limits_and_differ(gc):
    """At most six channels per set; the sets a sequence goes between differ in their first channels, so that `before`
    and `after` cannot give the same bytes; the streams hold what the trackers are asked to run."""
    for a, b in ((rc.IQ4_SIX_A, rc.IQ4_TWO_B), (rc.IQ4_TWO_A, rc.IQ4_SIX_B), (rc.RX_A, rc.RX_B)):
        assert len(a) <= 6 and len(b) <= 6 and len(set(a)) == len(a) and len(set(b)) == len(b)
        assert all(x != y for x, y in zip(a, b))
    assert len(rc.scen_specs("m26")) == 2 and len(rc.scen_specs("iq4")) == 6
    chans = rc.iq4_set(gc, rc.IQ4_SIX_A, 6)
    assert chans[0].ntap == 13 and chans[0].nsamp == rc.N4 and chans[0].nfreq == 15
    far = max(s["buffloc"] for s in rc.trk_states(chans, 1)) + (12 + 12 + 30 + 1) * (rc.N4 + 1)
    assert far < rc.TRK_PERIODS * rc.N4
    assert 50 + 700 * 5 + 61 * (rc.N4 + 1) < rc.TRK_PERIODS * rc.N4


def test_reconfiguring_calls_refuse_a_null_context(gc):
    L = gc.lib()
    one = (C.c_int * 1)(1)
    d = gc.Channel(1).desc()
    calls = [("ring_create", lambda: L.gnsscorr_ring_create(None, 1, 2, 1024, None), EINVAL),
             ("set_channels", lambda: L.gnsscorr_set_channels(None, 1, C.byref(d)), EINVAL),
             ("acq_set_coherent", lambda: L.gnsscorr_acq_set_coherent(None, 0, 1, one), EINVAL),
             ("acq_set_bitedge", lambda: L.gnsscorr_acq_set_bitedge(None, 0, 1, one), EINVAL),
             ("acq_set_refine", lambda: L.gnsscorr_acq_set_refine(None, 0, 1, one), EINVAL),
             ("rx_step", lambda: L.gnsscorr_rx_step(None, 1), ESTATE),
             ("rx_set", lambda: L.gnsscorr_rx_set(None, 0, 1), ESTATE),
             ("rx_status", lambda: L.gnsscorr_rx_status(None, None), ESTATE),
             ("rx_lock_set", lambda: L.gnsscorr_rx_lock_set(None, 0, 1, None), ESTATE),
             ("rx_lock_status", lambda: L.gnsscorr_rx_lock_status(None, None, None), ESTATE),
             ("spec_fetch", lambda: L.gnsscorr_spec_fetch(None, None, 0, None, 0, None, 0, None, 0), ESTATE)]
    for name, call, code in calls:
        assert call() == code, name
        assert name.encode() in L.gnsscorr_last_error(), (name, L.gnsscorr_last_error())
    assert L.gnsscorr_rx_start(None, 0) == EINVAL and L.gnsscorr_ring_wrpos(None, 1) == 0


def test_header_states_the_contracts():
    hdr = " ".join(open(os.path.join(ROOT, "include", "gnsscorr.h")).read().replace("*", " ").split())
    for sentence in ("re-creates the ring under them", "GNSSCORR_EINVAL naming the channel, with nothing touched",
                     "switches the schedule off", "until the next gnsscorr_rx_start",
                     "gnsscorr_spec_fetch returns GNSSCORR_ESTATE until the next gnsscorr_spec_run",
                     "keeps the count of its last run"):
        assert sentence in hdr, sentence


def test_freeze_and_diff_see_bits():
    a = dict(x=[np.array([1.0, np.nan, 0.0]), 3], y=dict(f=0.5))
    b = dict(x=[np.array([1.0, np.nan, 0.0]), 3], y=dict(f=0.5))
    rc.same(a, b)
    b["x"][0][2] = -0.0                                     # equal to np.array_equal, not to the bytes
    assert np.array_equal(a["x"][0][[0, 2]], b["x"][0][[0, 2]])
    assert rc.diff(a, b) == [".x[0]: 1 of 3 elements, first at (2,)"]
    with pytest.raises(AssertionError):
        rc.same(a, b)
    rc.differ(a, b)
    b["x"][0][2] = 0.0
    b["y"]["f"] = float("nan")
    assert len(rc.diff(a, b)) == 1 and rc.diff(a, b)[0].startswith(".y.f")
    assert rc.freeze(np.zeros(4, np.float32)) != rc.freeze(np.zeros(2, np.float64))     # the same bytes, another value
    s = np.zeros(2, dtype=[("p", "<f8"), ("q", "<i4")])
    t = s.copy()
    t["q"][1] = 7
    assert rc.diff(dict(s=s), dict(s=t)) == [".s: 1 of 2 elements, first at (1,)"]
