"""Acquisition over a channel list (gnsscorr_acq_run_subset) on every acquisition path (-m gpu): the 65536-point
kernel (acq_corr64: list entries in groups of 8), 16.368 Msps channels forced onto it by a 26 Msps ring, the
32768-point kernel (acq_corr: groups of GC_ACQ_G = 4, early stop by arrival counters) with channels decided at
middle iterations, grids of 71 / 13 / 9 bins and intg 10 / 3 / 1 in one engine, and sequences of lists on one
engine (the list cache).

Method.  The full run is held to the oracle with the bars of tests/test_gpu_acq_edges.py (its `_check`: integers
and buffloc exact, peakr / cn0 to 1e-4, every decision acq_cases.MARGIN from a tie or the threshold).  Every list is
then run on an engine of its own whose device buffers are poisoned before first use (Engine.debug_poison): rows,
arrival counters and results a faulty kernel leaves unwritten hold garbage there, not an earlier run's correct
values.  A listed channel's gnsscorr_acqres_t and its acq_power array must equal the full run's bit for bit, the
other rows must be zero and their power refused.  In the sequence test the engine under test is an ordinary one
that runs list after list, and each result must equal the fresh engine's for that list and write position."""
import struct

import numpy as np
import pytest

import acq_cases as ac
from test_gpu_acq_edges import _check, _fill, _pair

pytestmark = pytest.mark.gpu

ZERO_RES = dict(acqcodei=0, freqi=0, acqfreq=0.0, cn0=0.0, peakr=0.0, flagacq=0, iters=0, buffloc=0)
POISON = 0x5A


def _bits(r):
    """An acq_fetch row as bytes: equality that also holds NaNs to their bit pattern."""
    return struct.pack("<iidddiiQ", r["acqcodei"], r["freqi"], r["acqfreq"], r["cn0"], r["peakr"], r["flagacq"],
                       r["iters"], r["buffloc"])


def _fetch(engine, nch, chosen, gc):
    """Results of the last run, the power arrays of the listed channels; the others' power must be refused."""
    res = engine.acq_fetch()
    P = {}
    for i in range(nch):
        if i in chosen:
            P[i] = engine.acq_power(i)
        else:
            with pytest.raises(gc.GnsscorrError):
                engine.acq_power(i)
    return res, P


def _fresh(gc, setup, wrpos, chosen, nch):
    """The list on a new engine with poisoned buffers: (results, power arrays of the listed channels)."""
    e = gc.Engine(0)
    try:
        e.debug_poison(POISON)
        setup(e)
        e.acq_run(wrpos, channels=list(chosen))
        return _fetch(e, nch, chosen, gc)
    finally:
        e.close()


def _same_as_full(got, full, pfull, chosen, where):
    res, P = got
    for i, r in enumerate(res):
        want = full[i] if i in chosen else ZERO_RES
        assert _bits(r) == _bits(want), (where, list(chosen), i, r, want)
    assert sorted(P) == sorted(chosen), (where, chosen)
    for i in chosen:
        assert P[i].tobytes() == pfull[i].tobytes(), (where, list(chosen), i)


def _lists_against_full(gc, engine, setup, wrpos, full, lists, where):
    nch = len(full)
    pfull = {i: engine.acq_power(i) for i in range(nch)}
    for chosen in lists:
        assert len(set(chosen)) == len(chosen)
        _same_as_full(_fresh(gc, setup, wrpos, chosen, nch), full, pfull, chosen, where)


# ---- the 65536-point path --------------------------------------------------------------------------------------------
# case B searches 9 channels at 26 Msps and 8 at 20 Msps; the ninth at 20 Msps is one more absent PRN
B9 = {"26M_iq": ac.B_CHANS["26M_iq"], "20M_real_if4M": ac.B_CHANS["20M_real_if4M"] + [10]}


@pytest.mark.parametrize("shape", list(ac.B_SHAPES))
def test_lists_on_the_65536_point_path(gc, orc, synth, engine, shape):
    """acq_cases case B, 9 channels the oracle decides at iterations 1, several middle ones and never: lists of one
    channel, of 7, 8 and 9 (either side of acq_corr64's group of 8), the last channel alone and all in reverse."""
    f_sf, f_if, dtype = ac.B_SHAPES[shape]
    W, n = ac.case_b_span(gc, synth, shape)
    lead = 2 * n + 999
    stream = np.concatenate([ac.noise(lead, dtype, 31), W])
    g = 16 // dtype
    ringlen = -(-len(stream) // g) * g
    stream = _fill(stream, ringlen, dtype, 32)
    pairs = [_pair(gc, orc, p, dtype, f_sf, f_if, ac.B_GRID) for p in B9[shape]]
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    assert len(chans) == 9 and chans[0].nsamp > 16384

    def setup(e):
        e.ring_create(1, dtype, ringlen)
        e.ring_push_raw(1, stream, ringlen)
        e.set_channels(chans)

    setup(engine)
    wrpos = lead + 11 * n
    full, wants = _check(engine, orc, chans, ochs, [(stream, ringlen, wrpos)] * 9, wrpos, where=shape)
    print(f"lists, case B {shape}:", [(c.prn, w["flagacq"], w["iters"]) for c, w in zip(chans, wants)])
    assert len({w["iters"] for w in wants if w["flagacq"] and 2 <= w["iters"] <= 9}) >= 3
    assert not wants[8]["flagacq"] and wants[8]["iters"] == 10
    lists = [[4], [8, 1, 3, 5, 7, 0, 2], [1, 2, 3, 4, 5, 6, 7, 8], [3, 4, 5, 6, 7, 8, 0, 1, 2], [8],
             [8, 7, 6, 5, 4, 3, 2, 1, 0]]
    assert [len(x) for x in lists] == [1, 7, 8, 9, 1, 9]
    _lists_against_full(gc, engine, setup, wrpos, full, lists, shape)


def test_lists_with_mixed_rates_on_the_65536_point_path(gc, orc, synth, engine):
    """Ring 1 at 16.368 Msps beside ring 2 at 26 Msps (test_mixed_rates_force_65536's shape): acq_corr64 serves
    channels of nsamp 16368 and 26000 in one launch.  Lists of only the 16.368 Msps channels, only the 26 Msps
    channels, and one of each; every ring at its own write position."""
    Wa, na = ac.case_c_span(gc, synth, "16M_iq", 41)
    Wb, nb = ac.case_c_span(gc, synth, "26M_iq", 41)
    leada, leadb = 2 * na + 17, nb + 4000
    sa = np.concatenate([ac.noise(leada, 2, 81), Wa])
    sb = np.concatenate([ac.noise(leadb, 2, 82), Wb])
    rla, rlb = -(-len(sa) // 8) * 8, -(-len(sb) // 8) * 8
    sa, sb = _fill(sa, rla, 2, 83), _fill(sb, rlb, 2, 84)
    wa, wb = leada + 11 * na, leadb + 11 * nb
    pa = [_pair(gc, orc, p, 2, 16.368e6, 0.0, ac.C_GRID, ftype=1) for p in (ac.C_STRONG, ac.C_WEAK, ac.C_ABSENT)]
    pb = [_pair(gc, orc, p, 2, 26e6, 0.0, ac.C_GRID, ftype=2) for p in (ac.C_STRONG, ac.C_WEAK)]
    chans, ochs = [c for c, _ in pa + pb], [o for _, o in pa + pb]

    def setup(e):
        e.ring_create(1, 2, rla)
        e.ring_push_raw(1, sa[:wa], wa)
        e.ring_create(2, 2, rlb)
        e.ring_push_raw(2, sb[:wb], wb)
        e.set_channels(chans)

    setup(engine)
    rings = [(sa, rla, wa)] * 3 + [(sb, rlb, wb)] * 2
    full, wants = _check(engine, orc, chans, ochs, rings, 0, where="mixed rates")
    assert [w["flagacq"] for w in wants] == [1, 1, 0, 1, 1]
    assert 2 <= wants[1]["iters"] < 10 and 2 <= wants[4]["iters"] < 10
    _lists_against_full(gc, engine, setup, 0, full, [[0, 1, 2], [3, 4], [4, 3], [1, 4], [3, 2]], "mixed rates")


# ---- the 32768-point path --------------------------------------------------------------------------------------------
def _case_a_stream(gc, synth):
    """test_middle_iterations_32768's stream: two spans of 11 periods, other noise in each; the write positions."""
    n, L = ac.A_N, 11 * ac.A_N
    W1, W2 = (ac.case_a_span(gc, synth, s) for s in ac.A_SEEDS)
    lead, gap = 3 * n + 4321, 777
    stream = np.concatenate([ac.noise(lead, 2, 71), W1, ac.noise(gap, 2, 72), W2])
    ringlen = -(-len(stream) // 8) * 8
    return _fill(stream, ringlen, 2, 73), ringlen, lead + L, lead + L + gap + L


def test_lists_on_the_32768_point_path(gc, orc, synth, engine):
    """Case A, nine channels decided at iteration 1, at middle iterations and never: lists of 3, 4, 5 and 8.  The
    channel that runs all ten iterations stands once beside early-deciding channels in its group of 4 ([7, 8, 0, 1]:
    the group's workgroups go on for it after the others stopped) and once alone in a group ([0, 1, 2, 3, 8]).  iters
    of every listed channel as in the full run (part of the compared result; asserted by name as well)."""
    stream, ringlen, wr1, _ = _case_a_stream(gc, synth)
    pairs = [_pair(gc, orc, p, 2, ac.A_F_SF, 0.0) for p in ac.A_CHANS]
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]

    def setup(e):
        e.ring_create(1, 2, ringlen)
        e.ring_push_raw(1, stream, ringlen)
        e.set_channels(chans)

    setup(engine)
    full, wants = _check(engine, orc, chans, ochs, [(stream, ringlen, wr1)] * 9, wr1, where="case A lists")
    iters = [w["iters"] for w in wants]
    print("lists, case A:", [(c.prn, w["flagacq"], w["iters"]) for c, w in zip(chans, wants)])
    assert iters[7] == 1 and wants[7]["flagacq"] and iters[8] == 10 and not wants[8]["flagacq"]
    assert len({w["iters"] for w in wants if w["flagacq"] and 2 <= w["iters"] <= 9}) >= 3
    lists = [[2, 5, 7], [7, 8, 0, 1], [0, 1, 2, 3, 8], [8, 7, 6, 5, 4, 3, 2, 1]]
    assert [len(x) for x in lists] == [3, 4, 5, 8]
    assert min(iters[i] for i in (7, 0, 1)) < 10
    pfull = {i: engine.acq_power(i) for i in range(9)}
    for chosen in lists:
        got = _fresh(gc, setup, wr1, chosen, 9)
        assert [got[0][i]["iters"] for i in chosen] == [iters[i] for i in chosen], chosen
        _same_as_full(got, full, pfull, chosen, "case A")


def _case_e(gc, orc):
    pairs = [_pair(gc, orc, p, 2, ac.A_F_SF, 0.0, g) for p, g in ac.E_CHANS]
    return [c for c, _ in pairs], [o for _, o in pairs]


def test_lists_with_mixed_grids(gc, orc, synth, engine):
    """acq_cases.E_CHANS: grids of 71, 13 and 9 bins with intg 10, 3 and 1 in one engine, so maxfreq and maxintg exceed
    what most listed channels own.  Lists that leave out grid 0, that leave out the middle grid, that hold only the
    9-bin / intg 1 channel, and one channel of each grid in another order than the grids'."""
    n, L = ac.A_N, 11 * ac.A_N
    W = ac.case_a_span(gc, synth, ac.A_SEEDS[0])
    lead = n + 4444
    stream = np.concatenate([ac.noise(lead, 2, 41), W])
    ringlen = -(-len(stream) // 8) * 8
    stream = _fill(stream, ringlen, 2, 42)
    chans, ochs = _case_e(gc, orc)
    assert [c.nfreq for c in chans] == [71, 13, 13, 13, 9, 9] and [c.intg for c in chans] == [10, 3, 3, 3, 1, 1]

    def setup(e):
        e.ring_create(1, 2, ringlen)
        e.ring_push_raw(1, stream, ringlen)
        e.set_channels(chans)

    setup(engine)
    wrpos = lead + L
    full, wants = _check(engine, orc, chans, ochs, [(stream, ringlen, wrpos)] * 6, wrpos, where="mixed grid lists")
    assert [(w["flagacq"], w["iters"]) for w in wants] == [(1, 5), (1, 2), (0, 3), (0, 3), (1, 1), (0, 1)]
    lists = [[1, 2, 3, 4, 5], [0, 4, 5], [4], [5, 0, 2], [3]]
    _lists_against_full(gc, engine, setup, wrpos, full, lists, "mixed grids")


def test_list_sequences_on_one_engine(gc, orc, synth, engine):
    """The list cache ("the lists go up only when they change"): on one engine with the mixed grids of E_CHANS over
    case A's two spans -- A, then B disjoint from A, then A again at a later write position; the same list at two
    write positions; a list of the same length with other members (same grids, then other grids); a full run between
    two lists; a refused call (a duplicate entry; too few samples in the ring) between two runs of the same list.
    Every result equals a fresh, poisoned engine's for that list and position."""
    stream, ringlen, wr1, wr2 = _case_a_stream(gc, synth)
    chans, _ = _case_e(gc, orc)
    nch = len(chans)

    def setup(e):
        e.ring_create(1, 2, ringlen)
        e.ring_push_raw(1, stream, ringlen)
        e.set_channels(chans)

    setup(engine)
    cache = {}

    def run(chosen, wrpos):
        key = (tuple(chosen) if chosen is not None else None, wrpos)
        if key not in cache:
            cache[key] = _fresh(gc, setup, wrpos, chosen if chosen is not None else list(range(nch)), nch)
        engine.acq_run(wrpos, channels=chosen)
        got = _fetch(engine, nch, chosen if chosen is not None else list(range(nch)), gc)
        want = cache[key]
        for i in range(nch):
            assert _bits(got[0][i]) == _bits(want[0][i]), (key, i, got[0][i], want[0][i])
        assert sorted(got[1]) == sorted(want[1])
        for i in got[1]:
            assert got[1][i].tobytes() == want[1][i].tobytes(), (key, i)
        return got[0]

    A, B = [0, 1, 4], [2, 3, 5]
    r_a1 = run(A, wr1)
    run(B, wr1)
    r_a2 = run(A, wr2)                                          # A again, later
    assert [_bits(r) for r in r_a1] != [_bits(r) for r in r_a2]   # (the two spans give other results)
    run(A, wr1)                                                 # the same list at two write positions, back to back
    run([0, 1, 5], wr1)                                         # same length, same grids, another member
    run([0, 2, 5], wr1)
    run([1, 2, 5], wr1)                                         # same length, other grids (no 71-bin grid)
    run([5, 2, 1], wr1)                                         # the same members in another order
    run(None, wr2)                                              # a full run between two lists
    run([5, 2, 1], wr1)
    for bad, wp in (([5, 2, 2], wr1), ([0, 1, 4], 5 * ac.A_N), ([6], wr1), ([], wr1)):
        with pytest.raises(gc.GnsscorrError):
            engine.acq_run(wp, channels=bad)
        run([5, 2, 1], wr1)                                     # the same list after a refused call
    run([4], 2 * ac.A_N)                                        # (2 periods are enough for the intg 1 grid alone)
    run(A, wr2)
