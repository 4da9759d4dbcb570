"""Carrier frequency refinement (gnsscorr_acq_set_refine) on the host: the accuracy of the estimator
as tests/acq_fine_cases.py restates it, the margins that make q* an exact comparison for every scenario of
tests/test_gpu_acq_fine.py, and the interface.  No GPU.

Accuracy, with step = 1/(2 K ctime) = 1.953 Hz the estimator's grid at 1 ms:
  - noise-free spans (one satellite at amplitude 40, IQ and real samples, 4.092 and 2.048 Msps, nref 2 and 10, the
    offsets -90, -37, +13, +90 Hz): |finefreq - f_true| <= one step.  Observed: at most 1.28 Hz (+13 Hz at nref 2),
    0.67 Hz in every other case -- the carrier LUT's quantisation does not show at this resolution, so the bar of one
    step stands as it is;
  - 45 dB-Hz, seeds 0..3, the data bit flipped after the span's first refine period: |finefreq - f_true| <=
    1/(4 nref ctime), 125 Hz for nref 2 and 25 Hz for nref 10.  Observed: at most 68.2 Hz (nref 2) and 4.06 Hz (nref
    10); DESIGN.md 3.2e has the table.
"""
import ctypes as C
import os

import numpy as np
import pytest

import acq_fine_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPER = 11                   # periods of an accuracy span: lag + 10 refine periods fit


def _lone(gc, orc, synth, name, sat, nref, cn0=None, seed=0, flip=False):
    """The restatement over a span with `sat` alone, from the satellite's lag on, at the nearest bin centre of the
    scenario's grid for it: (finefreq - f_true, result)."""
    sc = fc.SCEN[name]
    chan = next(ch for ch in sc["chans"] if ch[0] == sat[0])
    c, o = fc.ec.pair(gc, orc, sc, chan)
    n = c.nsamp
    W = fc.lone_span(gc, synth, sc, sat, NPER, cn0=cn0, seed=seed, flip=sat[1] + n if flip else None)
    ft = fc.f_true(sc, sat[0])
    res = dict(flagacq=1, buffloc=sat[1], acqfreq=fc.nearest_bin(c, ft))
    assert 0 < abs(res["acqfreq"] - ft) <= 100.0
    r = fc.fine_freq(orc, o, W, len(W), res, nref)
    assert r["nref"] == nref and r["q"] == round((r["finefreq"] - res["acqfreq"]) * 2 * fc.K * c.ctime)
    return r["finefreq"] - ft, r, c


@pytest.mark.parametrize("name", fc.SMALL)
def test_noise_free_spans_within_one_step(gc, orc, synth, name):
    """Both data types and both small rates, every satellite of the scenario alone and free of noise: the estimate is
    within one step of the estimator's grid of the true frequency -- on the side of the bin centre the satellite is on,
    which pins the sign of rule 6 -- and the line is clean."""
    worst = 0.0
    for sat in fc.SCEN[name]["sats"]:
        for nref in (2, 10):
            err, r, c = _lone(gc, orc, synth, name, sat, nref)
            print(f"noise-free {name} prn {sat[0]} nref {nref}: q {r['q']} error {err:+.3f} Hz quality {r['quality']:.6f}")
            worst = max(worst, abs(err))
            assert abs(err) <= fc.step(c.ctime), (name, sat[0], nref, err)
            assert r["quality"] > 0.99 and r["gap"] > fc.GAP
    print(f"noise-free {name}: worst |error| {worst:.3f} Hz, step {fc.step(1e-3):.3f} Hz")


@pytest.mark.parametrize("nref", [2, 10])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_noisy_spans_on_the_right_lobe(gc, orc, synth, seed, nref):
    """45 dB-Hz, the data bit flipped after the first refine period (inside the span for nref 2 and 10 alike): the
    estimate lies within half the null-to-peak width of the squared line, 1/(4 nref ctime), of the true frequency."""
    for name in fc.SMALL:
        for sat in fc.SCEN[name]["sats"]:
            err, r, c = _lone(gc, orc, synth, name, sat, nref, cn0=45.0, seed=seed, flip=True)
            print(f"45 dB-Hz {name} prn {sat[0]} seed {seed} nref {nref}: error {err:+.2f} Hz quality {r['quality']:.3f}")
            assert abs(err) <= 1.0 / (4.0 * nref * c.ctime), (name, sat[0], seed, nref, err)


@pytest.mark.parametrize("name", sorted(fc.SCEN))
def test_margins_of_the_device_scenarios(gc, orc, synth, name):
    """Every scenario of tests/test_gpu_acq_fine.py, for both nref it is run with: the restated search acquires its
    satellites at a bin centre they are off, and the largest |Z[q]|^2 leads every other q by more than 1e-9 relative --
    fp64 sums of <= 20 terms differ by ~1e-15 between device and numpy, so q* is a safe exact comparison."""
    sc = fc.SCEN[name]
    W, pairs, wants = fc.scenario(gc, orc, synth, name)
    for (c, o), w in zip(pairs, wants):
        ft = fc.f_true(sc, c.prn)
        fc.ec.check_margins(w, (name, c.prn))           # the search itself is decided with room: the device's is this one
        assert bool(w["flagacq"]) == (ft is not None), (name, c.prn)
        if ft is not None:
            # off a bin centre and inside the estimator's unambiguous range, 1/(4 ctime) (a satellite 90 Hz off its
            # bin may be found in the neighbour, 110 Hz off: iq2's PRN 17 is)
            assert 0 < abs(w["acqfreq"] - ft) < 1.0 / (4.0 * c.ctime) and w["acqfreq"] in c.freq, (name, c.prn)
    for nref in fc.nrefs(sc):
        for (c, o), r in zip(pairs, fc.fine_all(orc, pairs, W, len(W), wants, nref)):
            ft = fc.f_true(sc, c.prn)
            if ft is None:
                assert r["nref"] == 0 and r["quality"] == 0.0 and not r["prompt"].any()
                continue
            print(f"{name} prn {c.prn} nref {nref}: q {r['q']} error {r['finefreq'] - ft:+.2f} Hz "
                  f"quality {r['quality']:.3f} gap {r['gap']:.3g}")
            assert r["gap"] > fc.GAP, (name, c.prn, nref, r["gap"])
            assert abs(r["finefreq"] - ft) <= 1.0 / (4.0 * nref * c.ctime), (name, c.prn, nref)
            assert np.abs(r["prompt"]).max() < 1 << 28


def test_margins_of_the_handover_signal(gc, orc, synth):
    """The same conditions for the signal the hand-over test searches and tracks: both satellites acquired off their
    bin centres with room, q* decided with a gap above 1e-9, the absent PRN not acquired."""
    sig = fc.handover_signal(gc, synth)
    pairs = fc.handover_pairs(gc, orc)
    wants = fc.ec.restate(orc, pairs, sig, len(sig), fc.HO_WRPOS)
    assert [bool(w["flagacq"]) for w in wants] == [True, True, False]
    fine = fc.fine_all(orc, pairs, sig, len(sig), wants, fc.HO_NREF)
    for (c, _), w, r, ft, nref in zip(pairs, wants, fine, fc.HO_DOP, fc.HO_NREF):
        fc.ec.check_margins(w, ("handover", c.prn))
        assert 0 < abs(w["acqfreq"] - ft) < 1.0 / (4.0 * c.ctime) and r["nref"] == nref
        if nref:
            print(f"handover prn {c.prn}: coarse {w['acqfreq'] - ft:+.1f} Hz, fine {r['finefreq'] - ft:+.2f} Hz, gap {r['gap']:.3g}")
            assert r["gap"] > fc.GAP and abs(r["finefreq"] - ft) <= 1.0 / (4.0 * nref * c.ctime)
    fc.ec.check_margins(wants[2], ("handover", "absent"))


def test_surface(gc):
    """The three entry points are exported and declared, the result struct is 24 bytes, GNSSCORR_FINE_BINS is the
    helpers' K, and set_refine on a null context is an error that needs no device."""
    L = gc.lib()
    hdr = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    for name in ("gnsscorr_acq_set_refine", "gnsscorr_acq_get_refine", "gnsscorr_acq_fetch_fine"):
        assert hasattr(L, name) and name in gc.EXPORTS_GNSSCORR and (name + "(") in hdr, name
    assert C.sizeof(gc.AcqFine) == 24 and [f[0] for f in gc.AcqFine._fields_] == ["finefreq", "quality", "q", "nref"]
    assert "#define GNSSCORR_FINE_BINS 256" in hdr and gc.FINE_BINS == fc.K == 256 and gc.MAXCOH == fc.MAXCOH
    one = (C.c_int * 1)(2)
    assert L.gnsscorr_acq_set_refine(None, 0, 1, one) != 0
    assert b"acq_set_refine" in L.gnsscorr_last_error()
    assert L.gnsscorr_acq_get_refine(None, 0, 1, one) != 0 and one[0] == 2
    assert L.gnsscorr_acq_fetch_fine(None, None, None) != 0
    assert gc.Channel(1, nref=4).nref == 4 and gc.Channel(1).nref == 0
