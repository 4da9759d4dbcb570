"""Bit-edge hypotheses for coherent groups (gnsscorr_acq_set_bitedge) on the host: that the restatement of their
semantics (tests/acq_edge_cases.py) is acq_coh_cases.coh_acq for estep = 0 and costs an unflipped satellite nothing, the
sensitivity claim behind the feature on the literal LUT path, that every scenario tests/test_gpu_acq_bitedge.py and
tests/test_gpu_acq_bitedge_positions.py run on the device is decided on the restatement with room, that a span moved in
its stream and ring is the same search, and that the library exports the entry points.  No GPU.

Figures (restatement, 4.092 Msps IQ, PRN 1 at +1000 Hz and lag 1234, sigma 8, intg 10, ncoh 10, +-5 kHz / 50 Hz, 36
dB-Hz, the data bit flipped at sample 1234 + 5 * 4092 of the span), seeds 0 / 1 / 2 / 3:
  estep 0: peak ratio 2.31 / 2.85 / 2.86 / 2.83 in bins 118 / 121 / 121 / 122: never acquired;
  estep 1: 3.61 / 3.65 / 3.57 / 4.69 at lag 1234, bin 120, edge 5: acquired, all four;
  estep 2 (4 and 6 straddle the edge): 2.80 / 2.56 / 2.86 / 3.00 (2.995): not acquired.
  Rows of the 201 whose two best hypotheses lie within MARGIN of each other: at most 4 (2 %), never the deciding one.
The scenarios of the device tests (peak ratio per group; smallest lag gap, row gap and gap between the deciding row's
two best hypotheses over the scenario's channels).  edges40 took seed 54: at seeds 4, 14, 24, 34 and 44 some layout of
it had a 9-bin channel with one row tied on its hypotheses (11 % of its rows) or the absent PRN's rows 3e-4 apart; the
others run on their first seed and C/N0.  Where the checked satellites' lags come from: acq_edge_cases.SCEN.
  edge36  estep 0 / 1 / 2: 2.858 / 3.568 (edge 5) / 2.858; gaps 0.033, 0.069, 0.178
  edges40 edge 1: 10.08, edge 9: 15.80, none: 17.14 (edge 0), flip 0.72 into period 4: 9.21 (edge 4, 1.9 % ahead of
          5), absent: 1.24; 0.157, 0.079, 0.019
  groups5 45 dB-Hz: 16.73 at group 1 (edge 3); 36.5 dB-Hz: 2.884 then 4.418 (rows of h 3 and h 0 added, edge 0);
          absent: 1.67, 1.90; 0.065, 0.068, 0.195
  step2   edge 4: 41.13 (edge 4); edge 5: 20.12 (edge 6, 1.2 % ahead of hypothesis 4); 0.367, 0.285, 0.012
  real    7.293 (edge 2); 0.171, 0.447, 0.698
  mixed   4.516 / 6.880 / 8.709 (edge 2) / 15.04 (edge 5); 0.010, 0.049, 0.547
The scenarios of tests/test_gpu_acq_bitedge_positions.py (asserted in test_figures_of_the_new_scenarios; no row of
any of them is tied).  Seeds 11 and 12 of odd and 21 to 27 of moved had a channel with one of its nine rows tied:
  odd     estep 3 / 4 / 9 on ncoh 10: 17.42 (edge 9) / 22.19 (edge 8) / 17.42 (edge 9); estep 4 on ncoh 5: 5.893 at
          group 1 (edge 4); absent: 1.312; 0.233, 0.037, 0.032 (0.340 over the acquired channels)
  two     40 dB-Hz: 1.40, 2.32, 3.54 (hypotheses 0, 0, 1; edge 1, iters 6); 46 dB-Hz: 10.71 at group 1 (edge 1);
          absent: 1.23, 1.04, 1.19, 1.08, 1.14; lag gap 0.038, row gap 0.0031, hypothesis gap 0.0094 (all the absent PRN's)
  twenty  26.0 (edge 19) / 17.04 (edge 10) / absent 1.678; hypothesis gaps 0.136 / 0.176 / 0.075
  moved   periods 0..10: 15.04 (edge 3) / 12.49 (0) / 17.16 (0) / 16.40 (1) / absent 1.525, hypothesis gaps >= 0.298, 0.123;
          periods 2..12: 17.35 (edge 1) / 19.66 (9) / 18.98 (0) / 16.25 (0) / absent 1.705, >= 0.282, 0.0082
The same scenarios away from the origin (rings that end inside the span, an odd offset, 2^32) give these figures again,
group by group (test_positions_reproduce_the_origin)."""
import ctypes as C
import os

import numpy as np
import pytest

import acq_cases as ac
import acq_coh_cases as cc
import acq_edge_cases as ec


@pytest.fixture(scope="module")
def scen(gc, orc, synth):
    return lambda name: ec.scenario(gc, orc, synth, name)


def test_estep0_restatement_is_coh_acq(gc, orc, synth):
    """estep = 0 through edge_acq: coh_acq bit for bit (results, every step, the power array), groups of 5 summed."""
    sc = ec.SCEN["groups5"]
    W = cc.make_span(gc, synth, sc)
    _, o = ec.pair(gc, orc, sc, (11, 400, 100, 10, 5, 0))
    got = ec.edge_acq(orc, o, W, len(W), len(W), 5, 0)
    want = cc.coh_acq(orc, o, W, len(W), len(W), 5)
    for k in ("flagacq", "iters", "buffloc", "acqcodei", "freqi", "acqfreq", "cn0", "peakr", "steps", "b0", "groups"):
        assert got[k] == want[k] or (k == "cn0" and np.isnan(got[k]) and np.isnan(want[k])), k
    assert want["groups"] == 2 and got["P"].tobytes() == want["P"].tobytes()
    assert got["edge"] == -1 and got["hs"] == [0] and all(np.all(h == 0) for h in got["hsel"])


def test_all_hypotheses_cost_an_unflipped_satellite_nothing(gc, orc, synth):
    """H = ncoh on a satellite without a bit edge: the deciding bin's row is coh_acq's, bit for bit, and with it the
    decision; edge 0.  (A per-cell maximum over the hypotheses would not have this property.)"""
    sc = cc.SCEN["iq10"]
    W = cc.make_span(gc, synth, sc)
    _, o = cc.pair(gc, orc, sc, (9, 200, 50, 10, 10))
    got = ec.edge_acq(orc, o, W, len(W), len(W), 10, 1)
    want = cc.coh_acq(orc, o, W, len(W), len(W), 10)
    assert got["hs"] == list(range(10)) and want["flagacq"] and got["flagacq"]
    fi = want["freqi"]
    assert got["freqi"] == fi and got["hsel"][0][fi] == 0 and got["edge"] == 0
    assert got["P"][fi].tobytes() == want["P"][fi].tobytes()
    for k in ("iters", "buffloc", "acqcodei", "acqfreq", "peakr", "cn0"):
        assert got[k] == want[k], k


def test_bit_edge_in_the_span_needs_the_hypotheses(gc, orc, synth, scen):
    """The claim the feature rests on, seeds 0..3: the 36 dB-Hz satellite whose bit flips on its fifth period boundary
    is never acquired without hypotheses, acquired at lag 1234 +- 1, bin 120, edge 5 with estep 1, and not acquired
    with estep 2, whose hypotheses 4 and 6 straddle the edge."""
    sc = dict(ec.SCEN["edge36"])
    prn, lag, dop, cn0, _, flip = sc["sats"][0]
    assert (prn, lag, dop, cn0, flip, sc["f_sf"]) == (1, 1234, 1000.0, 36.0, 1234 + 5 * 4092, 4.092e6)
    assert [c[4:] for c in sc["chans"]] == [(10, 0), (10, 1), (10, 2)] and sc["seed"] == 2
    pairs = scen("edge36")[1]
    assert all(c.nfreq == 201 for c, _ in pairs)
    jobs, seeds = [], (0, 1, 3)
    for seed in seeds:
        W = cc.make_span(gc, synth, dict(sc, seed=seed))
        # (an oracle channel of its own per job: they run side by side)
        jobs += [lambda W=W, ch=ch: ec.edge_acq(orc, ec.pair(gc, orc, sc, ch)[1], W, len(W), len(W), ch[4], ch[5])
                 for ch in sc["chans"]]
    out = ac.run_oracles(jobs)
    by_seed = {s: out[3 * i:3 * i + 3] for i, s in enumerate(seeds)}
    by_seed[2] = scen("edge36")[2]
    for seed in sorted(by_seed):
        r0, r1, r2 = by_seed[seed]
        print("seed %d: estep 0 peakr %.3f bin %d; estep 1 peakr %.3f lag %d bin %d edge %d; estep 2 peakr %.3f; tied "
              "rows %d / %d of 201" % (seed, r0["peakr"], r0["freqi"], r1["peakr"], r1["acqcodei"], r1["freqi"],
                                      r1["edge"], r2["peakr"], ec.tied_rows(r1).sum(), ec.tied_rows(r2).sum()))
        assert not r0["flagacq"] and r0["edge"] == -1
        assert r1["flagacq"] and abs(r1["acqcodei"] - lag) <= 1 and r1["freqi"] == 120 and r1["edge"] == 5
        assert r1["acqfreq"] == dop and r1["iters"] == 10
        assert not r2["flagacq"] and r2["edge"] == -1
        for r in (r0, r1, r2):
            ec.check_margins(r, ("edge36", seed, r["estep"]))


@pytest.mark.parametrize("name", list(ec.SCEN))
def test_every_scenario_is_decided_with_room(scen, name):
    """The conditions on the inputs of the device tests (acq_edge_cases.check_margins): lag MARGIN, row 2*MARGIN, peak
    ratio 3*MARGIN, the deciding row's hypotheses MARGIN apart, at most 5 % of the rows tied and never that one."""
    _, pairs, res = scen(name)
    for ch, r in zip(ec.SCEN[name]["chans"], res):
        assert not np.isnan(r["cn0"])
        ec.check_margins(r, (name, ch))
        assert r["groups"] == len(r["steps"]) and r["iters"] == (r["groups"] * ch[4] if r["flagacq"] else ch[3])
        print(name, ch, "acquired" if r["flagacq"] else "not acquired", "iters", r["iters"], "edge", r["edge"],
              "peak ratios", [round(s[0], 3) for s in r["steps"]], "gaps", [tuple(round(x, 4) for x in s[3:]) for s in r["steps"]],
              "hypothesis gaps", [round(float(g[s[2]]), 4) for g, s in zip(r["hgap"], r["steps"])],
              "tied rows", int(ec.tied_rows(r).sum()), "of", len(r["hgap"][0]))


def test_scenarios_are_what_the_device_tests_need(scen, gc, orc, synth):
    """Each scenario's satellites are found at the placed lag (+-1) and bin with the placed edge."""
    moved_at = ec.moved_origin(gc, orc, synth)

    def found(r, sat, ch, edge, iters):
        prn, hband, step = ch[:3]
        assert r["flagacq"] and abs(r["acqcodei"] - sat[1]) <= 1 and r["iters"] == iters, (ch, r["acqcodei"], r["iters"])
        assert r["freqi"] == hband // step + round(sat[2] / step) and r["edge"] == edge, (ch, r["freqi"], r["edge"])

    for name, want in (("edges40", [(1, 10), (9, 10), (0, 10), (4, 10), None]),     # (the flip lies 0.72 into period 4)
                       ("groups5", [(3, 5), (0, 10), None]),
                       # an edge between two hypotheses: 4 and 6 each get one period wrong; 6 leads by 1.2 % here
                       ("step2", [(4, 10), (6, 10)]),
                       ("real", [(2, 4)]),
                       ("mixed", [(-1, 1), (-1, 5), (2, 5), (5, 10)]),
                       # every edge on the last hypothesis of a step that does not divide ncoh
                       ("odd", [(9, 10), (8, 10), (9, 10), (4, 5), None]),
                       ("two", [(1, 6), (1, 2), None]),
                       ("twenty", [(19, 20), (10, 20), None]),
                       ("moved@11", [(3, 10), (0, 10), (0, 10), (1, 10), None]),
                       ("moved", [(1, 10), (9, 10), (0, 10), (0, 10), None])):
        sc = ec.SCEN[name.split("@")[0]]
        placed = {s[0]: s for s in sc["sats"]}
        results = moved_at[0] if name == "moved@11" else scen(name)[2]
        for ch, r, w in zip(sc["chans"], results, want):
            if w is None:
                assert not r["flagacq"] and r["edge"] == -1 and r["iters"] == ch[3], (name, ch)
            else:
                found(r, placed[ch[0]], ch, *w)
    # groups5: the first group chooses the edge, the second (every period negated alike) none; the weak satellite's
    # power is the sum of two differently chosen rows
    strong, late, _ = scen("groups5")[2]
    assert strong["hsel"][0][strong["freqi"]] == 3
    assert [int(h[late["freqi"]]) for h in late["hsel"]] == [3, 0] and late["steps"][0][0] < 3.0 < late["steps"][1][0]
    # mixed: the intg-10 channels' spans start 10 periods into the intg-20 channel's
    assert [r["b0"] for r in scen("mixed")[2]] == [10 * 4092] * 3 + [0]
    # odd: H = ceil(ncoh / estep), the last hypothesis the one a floor would drop
    assert [r["hs"] for r in scen("odd")[2]] == [[0, 3, 6, 9], [0, 4, 8], [0, 9], [0, 4], [0, 3, 6, 9]]
    # two: the smallest H; three differently chosen rows are summed, the third group decides.  twenty: the largest
    slow, fast, absent = scen("two")[2]
    assert slow["hs"] == [0, 1] and [int(h[slow["freqi"]]) for h in slow["hsel"]] == [0, 0, 1]
    assert [s[0] < 3.0 for s in slow["steps"]] == [True, True, False] and fast["groups"] == 1 and absent["groups"] == 5
    assert all(r["hs"] == list(range(20)) and r["groups"] == 1 for r in scen("twenty")[2])
    # moved: a span of 13 periods, the searches begin at its periods 0 and 2
    assert len(scen("moved")[0]) == 13 * 4092 and [[r["b0"] for r in rs] for rs in moved_at] == [[0] * 5, [2 * 4092] * 5]


PEAKR = {   # peak ratio per group of every channel, the figures of this module's docstring (to 0.5 %)
    "odd": [[17.4], [22.2], [17.4], [5.89], [1.31]],
    "two": [[1.40, 2.32, 3.54], [10.7], [1.227, 1.04, 1.185, 1.078, 1.136]],
    "twenty": [[26.0], [17.0], [1.68]],
    "moved@11": [[15.0], [12.5], [17.2], [16.4], [1.52]],
    "moved": [[17.4], [19.7], [19.0], [16.3], [1.70]],
}


def test_figures_of_the_new_scenarios(scen, gc, orc, synth):
    """The restatement's peak ratios of odd, two, twenty and both searches of moved are the recorded ones: a change of
    the synthesiser, of a seed or of the restatement is noticed here, not on the device."""
    for name, want in PEAKR.items():
        res = ec.moved_origin(gc, orc, synth)[0] if name == "moved@11" else scen(name)[2]
        for i, (r, w) in enumerate(zip(res, want)):
            got = [s[0] for s in r["steps"]]
            print(name, i, [round(g, 3) for g in got])
            assert len(got) == len(w) and all(abs(g - x) <= 0.005 * x + 0.005 for g, x in zip(got, w)), (name, i, got)


def test_moved_searches_two_positions_with_room(gc, orc, synth):
    """The 13-period span of `moved` searched at its periods 0..10 and 2..12: both decided with room, the edges where
    the flips were placed relative to each search (rule 6 of DESIGN.md 3.2d on the restatement), and the same two
    searches on the stream the device test pushes (5 periods and 123 samples of noise in front)."""
    sc = ec.SCEN["moved"]
    W, pairs, _ = ec.scenario(gc, orc, synth, "moved")
    first, second = ec.moved_origin(gc, orc, synth)
    assert [r["edge"] for r in first] == [3, 0, 0, 1, -1] and [r["edge"] for r in second] == [1, 9, 0, 0, -1]
    for k, res in enumerate((first, second)):
        for ch, r in zip(sc["chans"], res):
            ec.check_margins(r, ("moved", k, ch))
            print("moved", k, ch, "edge", r["edge"], "peak ratio", round(r["peakr"], 3), "hypothesis gap",
                  round(float(r["hgap"][-1][r["freqi"]]), 4))
        assert [ec.rule6(sc, ch, r, r["edge"], 0) for ch, r in zip(sc["chans"], res)] == \
            [["edge", "none", "none", "edge", None], ["edge", "edge", "none", "none", None]][k]
    stream, ringlen, wrpos = ec.moved_stream(gc, orc, synth)
    assert ringlen >= len(stream) == ec.MOVED_B0 + 13 * 4092 and wrpos == [ec.MOVED_B0 + 11 * 4092, len(stream)]
    buf = ac.ring_order(stream, ringlen, len(stream))
    for wp, ref in zip(wrpos, (first, second)):
        for w, r in zip(ec.restate(orc, pairs, buf, ringlen, wp), ref):
            ec.same_search(w, r, ec.MOVED_B0)


@pytest.mark.parametrize("name,layout", ec.POSITIONS, ids=["-".join(p) for p in ec.POSITIONS])
def test_positions_reproduce_the_origin(gc, orc, synth, name, layout):
    """The scenarios away from the origin -- a ring end inside the span, real samples at an odd offset, a span across
    2^32 -- are the same search on the same samples: every group's figures, hypotheses and edges are the origin's, the
    positions moved by where the span begins.  So room is inherited.  And rule 6 holds on the restatement there."""
    sc = ec.SCEN[name]
    W, pairs, ref = ec.scenario(gc, orc, synth, name)
    p = ec.position(gc, orc, synth, name, layout)
    n = pairs[0][0].nsamp
    assert p["wrpos"] - p["b0"] == len(W) and p["ringlen"] >= len(W)
    into = (-p["b0"]) % p["ringlen"]              # span sample at the ring's slot 0
    print(name, layout, "ringlen", p["ringlen"], "b0", p["b0"], "the ring ends %.3f periods into the span" % (into / n))
    if layout == "2^32":
        assert p["b0"] + 2 * n < 1 << 32 < p["b0"] + 5 * n
    else:
        assert 0 < into < len(W)
        want = {"3.5": 3.5, "7.5": 7.5, "odd": 2.5}.get(layout)
        assert want is None or 0 <= into - want * n <= 1
        assert layout not in ("exact", "odd") or p["b0"] % 2 == 1
    for w, r in zip(p["wants"], ref):
        ec.same_search(w, r, p["b0"])
    said = [ec.rule6(sc, ch, w, w["edge"], p["b0"]) for ch, w in zip(sc["chans"], p["wants"])]
    assert said == {"groups5": ["edge", "none", None], "odd": ["edge"] * 4 + [None], "real": ["edge"]}[name]


def test_rule6_on_the_origin_scenarios(scen):
    """Rule 6 of DESIGN.md 3.2d against the synthesiser on the restatement: every acquired channel of odd, two and
    twenty names the sample at which its satellite's bit was flipped."""
    for name, want in (("odd", ["edge"] * 4 + [None]), ("two", ["edge", "edge", None]),
                       ("twenty", ["edge", "edge", None])):
        sc = ec.SCEN[name]
        assert [ec.rule6(sc, ch, r, r["edge"], 0) for ch, r in zip(sc["chans"], scen(name)[2])] == want, name
    # and it tells an edge off by one hypothesis, or a position that forgot where the span begins
    sc, (r, *_) = ec.SCEN["odd"], scen("odd")[2]
    with pytest.raises(AssertionError):
        ec.rule6(sc, sc["chans"][0], r, r["edge"] - 3, 0)
    with pytest.raises(AssertionError):
        ec.rule6(sc, sc["chans"][0], r, r["edge"], 3 * 4092)
    assert ec.rule6(sc, sc["chans"][0], r, r["edge"], 123) is None      # (callers assert what rule 6 said)


def test_library_exports_and_mirror(gc):
    """The .so exports the three entry points, the mirror binds them, the result struct keeps its size, and without a
    context all three answer GNSSCORR_EINVAL (no device needed)."""
    L = gc.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gnsscorr.h")).read()
    for name in ("gnsscorr_acq_set_bitedge", "gnsscorr_acq_get_bitedge", "gnsscorr_acq_fetch_edge"):
        assert hasattr(L, name) and name in gc.EXPORTS_GNSSCORR and (name + "(") in hdr, name
    ip = C.POINTER(C.c_int)
    assert L.gnsscorr_acq_set_bitedge.argtypes == [C.c_void_p, C.c_int, C.c_int, ip]
    assert L.gnsscorr_acq_get_bitedge.argtypes == [C.c_void_p, C.c_int, C.c_int, ip]
    assert L.gnsscorr_acq_fetch_edge.argtypes == [C.c_void_p, ip]
    assert C.sizeof(gc.AcqRes) == 48
    one = (C.c_int * 1)(1)
    assert L.gnsscorr_acq_set_bitedge(None, 0, 1, one) == -1 and L.gnsscorr_acq_get_bitedge(None, 0, 1, one) == -1
    assert L.gnsscorr_acq_fetch_edge(None, one) == -1
    assert "buffloc + ((iters / ncoh - 1) * ncoh + edge) * nsamp" in hdr
    c = gc.Channel(1, f_sf=4.092e6, hband=5000, step=50, ncoh=10, estep=2)
    assert (c.ncoh, c.estep) == (10, 2) and gc.Channel(1).estep == 0
