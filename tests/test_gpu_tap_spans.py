"""The closed loop (gnsscorr_trk_run_loop) at wide tap spans on every front end, against the oracle (parity tests
proper, -m gpu).  Cases: tests/tap_span_cases.py; tests/test_tap_spans_host.py shows on the CPU which rung of the tail's
code ladder serves each of them -- the shape-specialised step, the walker because the step's pieces pass GC_NCODE, or
one or the other from period to period of one channel.

Bar, nothing new: sums, samples per period, remainders, filter-update flags, flagsync and decided bits bit for bit,
filter outputs to 1e-12 with teacher forcing (tests/test_gpu_loop.py: _check_against_oracle, _adopt), final state equal
to the oracle's; the batched tracker as tests/test_gpu_tracking.py."""
import numpy as np
import pytest

import tap_span_cases as tc
from test_gpu_loop import _check_against_oracle
from test_gpu_loop_mixed import _check_final
from test_gpu_tracking import _oracle_run, _setup

pytestmark = pytest.mark.gpu


def _load(engine, sc):
    engine.ring_create(1, sc["case"]["dtype"], sc["nsamples"])
    engine.ring_push_raw(1, sc["data"], sc["nsamples"])
    engine.set_channels(sc["chans"])
    engine.trk_set_state(sc["states"])
    engine.loop_set([engine.loop_state(i, **nav) for i, nav in enumerate(sc["nav"])])


def _run_case(gc, orc, engine, case, flagsync):
    """4 channels x 40 periods in two runs (23 + 17) against the oracle's step, then the final state."""
    sc = tc.scene(gc, orc, case, flagsync)
    _load(engine, sc)
    done = 0
    for nrun in tc.CHUNKS:
        _check_against_oracle(orc, engine, sc["ochs"], sc["ring"], sc["bufflocs"], nrun, sc["ntap"], done=done, tol=1e-12)
        done += nrun
    _check_final(engine, sc["ochs"], sc["bufflocs"], sc["ntap"])


@pytest.mark.parametrize("flagsync", [0, 1])
@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c["id"])
def test_closed_loop_tap_span(gc, orc, engine, case, flagsync):
    """Every row of tap_span_cases.ROWS -- int8 IQ at 16.368, 4.092, 2.048, 8.1838 and 26 Msps, real samples at 20 Msps
    on a 4 MHz IF -- at outermost taps on either side of the span where the code step's pieces stop fitting the table,
    on it (2.048 Msps: 14; 20 Msps: 31 and 32, where it changes from period to period) and at 64 samples; seeded int8
    noise, before nav-bit sync (one period per step) and after (intervals of up to ten periods: table tasks of several
    periods per launch)."""
    _run_case(gc, orc, engine, case, flagsync)


def test_closed_loop_state_dependent_case_on_a_poisoned_engine(gc, orc):
    """20 Msps, 32 samples, after nav-bit sync -- about half of a channel's periods on either rung -- on a fresh engine
    whose buffers start out as 0xA5."""
    eng = gc.Engine(0)
    try:
        eng.debug_poison(0xA5)
        _run_case(gc, orc, eng, tc.BY_ID["real20_span32"], 1)
    finally:
        eng.close()


# One engine, one corrn (set_channels takes one CORRN per receiver): three-tap channels whose pair lies 64 samples
# out (the walker serves: the step's 60 pieces do not fit), 2 (the step on claims, tail class 0), 18 -- the span of the
# shipped 13-tap layout -- (class 2) and 8 (class 1); every rung of the tail's ladder in one launch.
MIXED_SPANS = (64, 2, 18, 8)


def _mixed_scene(gc, orc, flagsync, only=None):
    """The mixed engine's scene, or (only = i) channel i of it alone: same samples, same start state."""
    case = dict(tc.BY_ID["iq16_span64"], seed=6418)
    sc = tc.scene(gc, orc, case, flagsync, taps=(1, 1, 1))
    for i, span in enumerate(MIXED_SPANS):
        c, o = sc["chans"][i], sc["ochs"][i]
        sc["chans"][i] = gc.Channel(c.prn, dtype=2, f_if=0.0, f_sf=case["f_sf"], corrn=1, corrd=span, corrp=span)
        o2 = orc.make_chan(c.prn, dtype=2, f_sf=case["f_sf"], f_if=0.0, corrn=1, corrd=span, corrp=span)
        o2.acq.acqfreq = o.acq.acqfreq
        o2.carrfreq, o2.codefreq, o2.remcode, o2.remcarr = o.carrfreq, o.codefreq, o.remcode, o.remcarr
        o2.flagsync, o2.synci, o2.cnt = o.flagsync, o.synci, o.cnt
        sc["ochs"][i] = o2
    assert [int(c.corrp[-1]) for c in sc["chans"]] == list(MIXED_SPANS)
    if only is not None:
        for k in ("chans", "ochs", "states", "bufflocs", "nav"):
            sc[k] = [sc[k][only]]
    return sc


def _mixed_run(orc, engine, sc):
    """The two runs against the oracle; -> everything the engine returned, as bytes / plain values."""
    _load(engine, sc)
    out, done = [], 0
    for nrun in tc.CHUNKS:
        _check_against_oracle(orc, engine, sc["ochs"], sc["ring"], sc["bufflocs"], nrun, 3, done=done, tol=1e-12)
        II, QQ, ns = engine.trk_fetch()
        log, ndone = engine.trk_fetch_log()
        out.append((II, QQ, ns, log, ndone))
        done += nrun
    _check_final(engine, sc["ochs"], sc["bufflocs"], 3)
    return out, engine.trk_get_state()


@pytest.mark.parametrize("flagsync", [0, 1])
def test_closed_loop_mixed_spans_in_one_engine(gc, orc, engine, flagsync):
    """Outermost taps at 64, 2, 18 and 8 samples side by side at 16.368 Msps: against the oracle, and every channel bit
    for bit -- sums, samples, log rows, final state -- what the same channel gives alone on a fresh engine."""
    got, fin = _mixed_run(orc, engine, _mixed_scene(gc, orc, flagsync))
    for i in range(len(MIXED_SPANS)):
        alone = gc.Engine(0)
        try:
            ref, rfin = _mixed_run(orc, alone, _mixed_scene(gc, orc, flagsync, only=i))
        finally:
            alone.close()
        for (II, QQ, ns, log, ndone), (rII, rQQ, rns, rlog, rndone) in zip(got, ref):
            for u, v in ((II, rII), (QQ, rQQ), (ns, rns), (log, rlog), (ndone, rndone)):
                assert u[i:i + 1].tobytes() == v.tobytes(), (i, MIXED_SPANS[i])
        assert fin[i] == rfin[0], (i, MIXED_SPANS[i])


@pytest.mark.parametrize("row", sorted(tc.ROWS))
def test_batched_tracker_at_64_samples(gc, orc, engine, row):
    """trk_run on every front end of the table with 33 taps out to 64 samples: two batches of three periods against
    orc_sdrtracking, as tests/test_gpu_tap_sets.py::test_trk_tap_bucket_matches_oracle."""
    r = tc.ROWS[row]
    nsamples = tc.ring_samples(r["nsamp"], 6)
    data, chans, states, ochs = _setup(gc, orc, engine, r["dtype"], r["f_if"], *tc.TAPS64_BATCH, prns=[1, 7, 13, 32],
                                       nsamples=nsamples, seed=6400 + r["nsamp"] % 100, buffloc0=70, f_sf=r["f_sf"])
    assert chans[0].ntap == 33 and int(chans[0].corrp[-1]) == 64 and chans[0].nsamp == r["nsamp"]
    oII, oQQ, ons, ofin = _oracle_run(orc, ochs, states, data, nsamples, nsamples, 6)
    for b in range(2):
        engine.trk_run(3)
        II, QQ, ns = engine.trk_fetch()
        sl = slice(3 * b, 3 * b + 3)
        assert np.array_equal(ns, ons[:, sl]), (row, b)
        assert np.array_equal(II, oII[:, sl]) and np.array_equal(QQ, oQQ[:, sl]), (row, b)
    for a, o in zip(engine.trk_get_state(), ofin):
        assert a["remcode"] == o["remcode"] and a["remcarr"] == o["remcarr"] and a["buffloc"] == o["buffloc"], row
