"""Bit-edge hypotheses (gnsscorr_acq_set_bitedge) off the span origin and at odd edge steps, on the
device against the restatement tests/acq_edge_cases.py::edge_acq (parity tests proper, -m gpu).  What
tests/test_gpu_acq_bitedge.py leaves open, its ring being the span itself: edge steps that do not divide ncoh (H =
ceil(ncoh / estep), the edge on the last hypothesis), the ends of the range (ncoh 2; ncoh 20 = GNSSCORR_MAXCOH with 20
hypotheses), spans that begin anywhere in a stream with the ring's end inside a negated window, real samples at an odd
offset, a span across sample 2^32, two searches at two positions on one engine, the hand-over from such a position, and
rule 6 (where the data changes sign) held against where the synthesiser flipped the bit.  tests/test_acq_edge_host.py
shows on the host that every scenario is decided with room and that the moved spans are the same searches.

Bars, those of tests/test_gpu_acq_bitedge.py and none new: decisions and edges identical to the restatement's, peakr and
cn0 to 1e-4, acq_power element-wise to acq_cases.POWER_TOL x the row's noise mean against edge_power_td over the ring
the device holds, rows tied on their hypotheses left out (none is, in these scenarios).

Measured on the MI355X (every test prints its largest ratio |dP| / mean), the largest element-wise
power ratio per test: odd 4.5e-5, two 2.2e-5, twenty 7.2e-5 (40 dB-Hz, one group of 20); groups5 at 3.5 / 7.5 periods /
the exact ring / 2^32 2.6e-5 each (the origin's samples, the origin's figure), odd at 3.5 periods 4.5e-5, real samples
4.8e-5; moved 5.4e-5.  The device agreed with the restatement in all of them.  The file runs in about 4 s."""
import pytest

import acq_cases as ac
import acq_edge_cases as ec
import test_gpu_acq_bitedge as tb
from test_gpu_acq_bitedge import _check_power, _check_results, _granule, _scenario_on_engine
from test_gpu_positions import high_ring

pytestmark = pytest.mark.gpu

T32 = 1 << 32


def _largest(where, since):
    print(f"largest element-wise power ratio in {where}: {max(tb._ratios[since:]):.3g}")


def _rule6(sc, res, edge, w0, want, where):
    """Rule 6 on the device's fetched numbers, and that it spoke about the channels it should."""
    said = [ec.rule6(sc, ch, r, e, w0) for ch, r, e in zip(sc["chans"], res, edge)]
    assert said == want, (where, said)


# ---- 1. edge steps that do not divide ncoh; the ends of the range --------------------------------------------------
def test_steps_that_do_not_divide_ncoh(gc, orc, synth, engine):
    """estep 3, 4 and 9 on ncoh 10 and 4 on ncoh 5: H = 4, 3, 2, 2 = ceil(ncoh / estep), every acquired channel's edge
    on the last hypothesis (9, 8, 9, 4); an absent PRN with four."""
    since = len(tb._ratios)
    chans, res, edge, wants = _scenario_on_engine(engine, gc, orc, synth, "odd", power=(0, 1, 2, 3))
    assert engine.acq_get_bitedge() == [3, 4, 9, 4, 3] and [c.ncoh for c in chans] == [10, 10, 10, 5, 10]
    assert edge == [9, 8, 9, 4, -1] and [(r["flagacq"], r["iters"]) for r in res] == [(1, 10)] * 3 + [(1, 5), (0, 10)]
    _rule6(ec.SCEN["odd"], res, edge, 0, ["edge"] * 4 + [None], "odd")
    _largest("odd", since)


def test_groups_of_two(gc, orc, synth, engine):
    """ncoh 2, estep 1: the smallest H, five groups of two slots.  The 40 dB-Hz satellite passes at group 3, its power
    the sum of the rows of hypotheses 0, 0 and 1; the strong one at group 1; the absent PRN runs all five."""
    since = len(tb._ratios)
    chans, res, edge, wants = _scenario_on_engine(engine, gc, orc, synth, "two", power=(0, 1))
    assert [(r["flagacq"], r["iters"]) for r in res] == [(1, 6), (1, 2), (0, 10)] and edge == [1, 1, -1]
    assert [int(h[wants[0]["freqi"]]) for h in wants[0]["hsel"]] == [0, 0, 1]
    _rule6(ec.SCEN["two"], res, edge, 0, ["edge", "edge", None], "two")
    _largest("two", since)


def test_twenty_periods_twenty_hypotheses(gc, orc, synth, engine):
    """ncoh 20 = GNSSCORR_MAXCOH, estep 1: H = maxslot = 20 on a poisoned engine (X is sized by maxslot), a carrier walk
    of 21 periods; an edge at 19, all windows but one negated, and one at 10."""
    since = len(tb._ratios)
    engine.debug_poison(0xA5)
    chans, res, edge, wants = _scenario_on_engine(engine, gc, orc, synth, "twenty", power=(0, 1))
    assert [(c.ncoh, c.estep, c.intg) for c in chans] == [(20, 1, 20)] * 3
    assert [(r["flagacq"], r["iters"]) for r in res] == [(1, 20), (1, 20), (0, 20)] and edge == [19, 10, -1]
    _rule6(ec.SCEN["twenty"], res, edge, 0, ["edge", "edge", None], "twenty")
    _largest("twenty", since)


# ---- 2. positions: the span anywhere in a stream, the ring's end inside it, 2^32 -----------------------------------
def _position_on_engine(engine, gc, orc, synth, name, layout):
    """The ring as acq_edge_cases.position lays it out, the channels set and the search run: (chans, ochs, p)."""
    sc = ec.SCEN[name]
    _, pairs, _ = ec.scenario(gc, orc, synth, name)
    p = ec.position(gc, orc, synth, name, layout)
    if p["K"] is None:
        engine.ring_create(1, sc["dtype"], p["ringlen"])
        ac.push_wrapping(engine, 1, p["stream"], p["wrpos"], p["ringlen"])
    else:
        assert high_ring(engine, 1, sc["dtype"], p["stream"], p["ringlen"], p["K"]) == p["wrpos"]
    assert engine.ring_wrpos(1) == p["wrpos"] and p["ringlen"] == _granule(p["ringlen"], sc["dtype"])
    chans = [c for c, _ in pairs]
    engine.set_channels(chans)
    assert engine.acq_get_bitedge() == [c.estep for c in chans]
    engine.acq_run(p["wrpos"])
    return chans, [o for _, o in pairs], p


POWER = {("groups5", "3.5"): (0, 1), ("groups5", "7.5"): (0, 1), ("groups5", "exact"): (0, 1),
         ("odd", "3.5"): (0, 1, 2, 3), ("real", "odd"): (0,), ("groups5", "2^32"): (0,)}


@pytest.mark.parametrize("name,layout", ec.POSITIONS, ids=["-".join(p) for p in ec.POSITIONS])
def test_span_off_the_origin(gc, orc, synth, engine, name, layout):
    """stream = noise(b0) ++ span, pushed in pieces; the restatement reads the ring order the device holds.
    groups5 (ncoh 5, edge 3 in group 0) on rings of 13 periods that end 3.5 periods into the span -- inside window 3 of
    group 0, the first negated window of the winning hypothesis -- and 7.5 periods into it, inside group 1, and on a ring
    of exactly the span after an odd b0; odd (edge 9, steps that do not divide) at 3.5 periods; real samples (dtype 1,
    nsamp 16368, H = 4) on a ring that ends at an odd offset inside window 2; groups5 with 2^32 between its windows 2
    and 4 of group 0."""
    since = len(tb._ratios)
    where = f"{name} {layout}"
    sc = ec.SCEN[name]
    chans, ochs, p = _position_on_engine(engine, gc, orc, synth, name, layout)
    n, b0 = chans[0].nsamp, p["b0"]
    assert b0 > 0 and all(w["b0"] == b0 for w in p["wants"])
    res, edge = _check_results(engine, chans, p["wants"], where)
    if layout == "2^32":
        assert b0 + 2 * n < T32 < b0 + 5 * n and res[0]["buffloc"] < T32 < res[2]["buffloc"] == b0 + 10 * n
    want = {"groups5": ([3, 0, -1], [(1, 5), (1, 10), (0, 10)], ["edge", "none", None]),
            "odd": ([9, 8, 9, 4, -1], [(1, 10)] * 3 + [(1, 5), (0, 10)], ["edge"] * 4 + [None]),
            "real": ([2], [(1, 4)], ["edge"])}[name]
    assert edge == want[0] and [(r["flagacq"], r["iters"]) for r in res] == want[1]
    for i in POWER[(name, layout)]:
        _check_power(engine, orc, i, chans[i], ochs[i], p["wants"][i], (p["buf"], p["ringlen"]), where)
    _rule6(sc, res, edge, b0, want[2], where)
    _largest(where, since)


# ---- 3. two searches at two positions on one engine ----------------------------------------------------------------
def test_two_searches_two_positions_one_engine(gc, orc, synth, engine):
    """A 13-period span behind 5 periods and 123 samples of noise, the ring holding all of it; intg 10, ncoh 10, estep 1
    searches that end at the span's period 11 and then at 13, without set_channels in between: the edges move with
    the search ([3, 0, 0, 1, -1], then [1, 9, 0, 0, -1]).  Then the first position again, bit for bit its first
    answer, and the second on a fresh poisoned engine, bit for bit the first engine's."""
    since = len(tb._ratios)
    sc = ec.SCEN["moved"]
    _, pairs, _ = ec.scenario(gc, orc, synth, "moved")
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    stream, ringlen, wrpos = ec.moved_stream(gc, orc, synth)
    buf = ac.ring_order(stream, ringlen, len(stream))
    n, w0 = chans[0].nsamp, ec.MOVED_B0

    def load(e):
        e.ring_create(1, 2, ringlen)
        ac.push_wrapping(e, 1, stream, len(stream), ringlen)
        assert e.ring_wrpos(1) == len(stream)
        e.set_channels(chans)

    def answer(e):
        return e.acq_fetch(), e.acq_fetch_edge(), [e.acq_power(i).tobytes() for i in range(len(chans))]

    load(engine)
    got = []
    for k, (wp, edges, said) in enumerate(zip(wrpos, ([3, 0, 0, 1, -1], [1, 9, 0, 0, -1]),
                                              (["edge", "none", "none", "edge", None],
                                               ["edge", "edge", "none", "none", None]))):
        wants = ec.restate(orc, pairs, buf, ringlen, wp)
        assert [w["b0"] for w in wants] == [w0 + 2 * k * n] * 5
        engine.acq_run(wp)
        res, edge = _check_results(engine, chans, wants, f"moved {k}")
        assert edge == edges and [r["flagacq"] for r in res] == [1, 1, 1, 1, 0]
        for i in (0, 1, 3):
            _check_power(engine, orc, i, chans[i], ochs[i], wants[i], (buf, ringlen), f"moved {k}")
        _rule6(sc, res, edge, w0, said, f"moved {k}")
        got.append(answer(engine))
    assert got[0][0] != got[1][0] and got[0][2] != got[1][2]
    engine.acq_run(wrpos[0])                                # back: nothing of the second search is left
    assert answer(engine) == got[0]
    other = gc.Engine(0)
    try:
        other.debug_poison(0xA5)
        load(other)
        other.acq_run(wrpos[1])                             # and the second needed nothing of the first
        assert answer(other) == got[1]
    finally:
        other.close()
    _largest("moved", since)


# ---- 4. hand-over from a span that does not begin at 0 -------------------------------------------------------------
def test_handover_from_a_wrapped_span(gc, orc, synth, engine):
    """groups5 on the ring that ends 3.5 periods into the span: trk_start_from_acq and loop_start_from_acq leave what
    acq_start_state defines for the restated result -- carrfreq = acqfreq, codefreq = crate, zero remainders, the
    restatement's buffloc, b0 included -- on the acquired channels, and the unacquired channel's state as set."""
    chans, _, p = _position_on_engine(engine, gc, orc, synth, "groups5", "3.5")
    wants = p["wants"]
    assert [w["flagacq"] for w in wants] == [1, 1, 0] and all(w["buffloc"] > p["b0"] > 0 for w in wants)
    keep = [dict(carrfreq=300.0 * i, codefreq=c.crate + 1.0, remcode=0.5, remcarr=1.0, buffloc=4321 * (i + 1))
            for i, c in enumerate(chans)]
    want_state = [dict(carrfreq=w["acqfreq"], codefreq=c.crate, remcode=0.0, remcarr=0.0, buffloc=w["buffloc"])
                  if w["flagacq"] else k for c, w, k in zip(chans, wants, keep)]
    engine.trk_set_state(keep)
    engine.loop_set([engine.loop_state(i, 1.0 + i, flagsync=1, synci=3, cnt=100 + i) for i in range(3)])
    engine.acq_run(p["wrpos"])
    _check_results(engine, chans, wants, "handover")
    engine.trk_start_from_acq()
    assert engine.trk_get_state() == want_state
    engine.trk_set_state(keep)
    engine.loop_start_from_acq()
    assert engine.trk_get_state() == want_state
    for i, (ls, w) in enumerate(zip(engine.loop_get(), wants)):
        if w["flagacq"]:
            assert (ls.acqfreq, ls.cnt, ls.flagsync, ls.prn) == (w["acqfreq"], 0, 0, chans[i].prn), i
        else:
            assert (ls.acqfreq, ls.cnt, ls.flagsync) == (1.0 + i, 100 + i, 1), i
