"""The scenarios of tests/test_gpu_period_edges.py on the oracle alone (tests/period_edge_cases.py): the restated
segment geometry gives the boundaries the cases are named after, every tracking scene's periods lie on the side of its
boundary that the case is about, the int32 bound of the largest sum holds, and every acquisition scenario is decided
where it was placed, with room.  No GPU."""
import numpy as np
import pytest

import acq_cases as ac
import acq_fine_cases as fc
import period_edge_cases as pe


# ---- geometry --------------------------------------------------------------------------------------------------------
def test_restated_nseg_gives_the_boundaries():
    """nseg rises at 24446 + 24576 (k - 2) samples for real and 24461 + 24576 (k - 2) for IQ samples, k = 2 .. 11; at
    262144 samples it is 11 and every workgroup runs GC_MAXR rounds; the lengths the old suite ran stop at nseg 2."""
    for dtype, first in ((1, 24446), (2, 24461)):
        for k in range(2, 12):
            n = pe.first_nsamp(dtype, k)
            assert n == first + 24576 * (k - 2), (dtype, k, n)
            assert pe.nseg(dtype, n - 1) == k - 1 and pe.nseg(dtype, n) == k
        assert pe.first_nsamp(dtype, 12) == pe.NSAMP_MAX + 1
        assert pe.nseg(dtype, pe.NSAMP_MAX) == 11 and pe.rounds_per_seg(dtype, pe.NSAMP_MAX) == pe.GC_MAXR
        assert pe.rounds(dtype, pe.NSAMP_MAX) == 257
        assert [pe.nseg(dtype, n) for n in (2048, 4092, 8183, 16368, 20000, 26000)] == [1, 1, 1, 1, 1, 2]
        names = dict(pe.trk_lengths(dtype))
        assert [pe.nseg(dtype, names[k]) for k in ("one_sample_per_chip", "last_nseg1", "first_nseg2", "acq_limit",
                                                   "last_nseg2", "first_nseg3", "table_65000", "no_table_65535",
                                                   "no_table_65536", "nseg6_131072", "nseg11_262144")] == \
            [1, 1, 2, 2, 2, 3, 3, 3, 3, 6, 11]
    assert dict(pe.trk_lengths(1))["first_nseg2"] == 24446 and dict(pe.trk_lengths(1))["first_nseg3"] == 49022
    assert dict(pe.trk_lengths(2))["first_nseg2"] == 24461 and dict(pe.trk_lengths(2))["first_nseg3"] == 49037
    # a 2048-sample channel beside a 262144-sample one: its period fits the first of the context's eleven segments
    for dtype in (1, 2):
        rgrp = pe.GC_PS_WLANES * pe.nit(dtype)
        per_seg = rgrp * pe.rounds_per_seg(dtype, pe.NSAMP_MAX)
        assert pe.groups(dtype, pe.SHORT_NSAMP + 100) <= per_seg


def test_int32_bound_of_the_largest_sum(orc):
    """(262144 + 100) x 128 x max(|cos32| + |sin32|) < 2^31, from the table in gnsscorr_lut.h, which is the oracle's."""
    cos32, sin32 = pe.header_lut()
    ocos, osin = np.zeros(32, np.int16), np.zeros(32, np.int16)
    orc.lib().orc_carrier_lut(ocos.ctypes.data, osin.ctypes.data)
    assert np.array_equal(cos32, ocos) and np.array_equal(sin32, osin)
    assert int(np.max(np.abs(cos32) + np.abs(sin32))) == 46 and cos32[4] == sin32[4] == 23
    bound = pe.accumulator_bound(cos32, sin32)
    assert bound == 262244 * 128 * 46 and bound < 2 ** 31
    assert (pe.NSAMP_MAX + 100) * 128 * 47 < 2 ** 31 <= (pe.NSAMP_MAX + 100) * 128 * 64     # (the room there is)


# ---- tracking scenes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 2])
def test_tracking_lengths_land_on_their_side(gc, orc, dtype):
    """Every length's six periods per channel: the library's and the oracle's nsamp are the target, no period outruns
    the nsamp + 100 samples the segments are sized for, the replica positions n + 2 smax stay below 65535 up to 65000
    samples and reach it from 65535 samples on in every period that is not cut by its start phase; the channels whose
    code ends on an edge are there."""
    for name, nsamp in pe.trk_lengths(dtype):
        sc = pe.length_scene(gc, orc, dtype, nsamp)
        ons, nt = sc["ons"], pe.nt(sc)
        assert ons.shape[1] == pe.NPER and ons.max() <= nsamp + 1 and ons[:, 1:].min() >= nsamp - 1, (name, ons)
        assert all(st["buffloc"] % 8 for st in sc["states"][1:]) and any(st["remcode"] for st in sc["states"])
        if nsamp <= 65000:
            assert nt.max() < pe.NT_LIMIT, name
        elif nsamp in (65535, 65536):
            assert nt[:, 1:].min() >= pe.NT_LIMIT and sc["smax"] == 6, name
            # a closing chip edge beyond 65535 in at least two channels
            assert sum(pe.tail_edge(c.code) for c in sc["chans"]) >= 2, name
        print(f"dtype {dtype} {name}: nsamp {nsamp} nseg {pe.nseg(dtype, nsamp)} periods {ons.min()}..{ons.max()}")


@pytest.mark.parametrize("dtype", [1, 2])
def test_straddle_changes_sides_inside_a_batch(gc, orc, dtype):
    sc = pe.straddle_scene(gc, orc, dtype)
    nt = pe.nt(sc)
    # channel 2: a table for the first period only; the later ones end on an edge that starts beyond 65535
    assert nt[2, 0] == 65531 and nt[2, 1:].min() >= 65543 and pe.tail_edge(sc["chans"][2].code)
    assert sc["ons"][2, 1:].min() + sc["smax"] > 65535
    # channel 3: 65534 and 65535 replica positions in turn, both inside each batch of three
    for b in range(2):
        assert sorted(set(nt[3, 3 * b + (b == 0):3 * b + 3].tolist())) == [65534, 65535], nt[3]
    assert nt[3, 0] < pe.NT_LIMIT


@pytest.mark.parametrize("dtype", [1, 2])
def test_codes_with_and_without_a_table(gc, orc, dtype):
    sc = pe.codes_scene(gc, orc, dtype)
    edges = [pe.code_edges(c.code) for c in sc["chans"]]
    assert edges[0] == 1022 > pe.GC_EDGTAB and edges[1] == 0 and 0 < edges[2] <= pe.GC_EDGTAB - 64
    assert pe.nt(sc).max() < pe.NT_LIMIT and pe.nseg(dtype, pe.CODES_NSAMP) == 1
    # the codes the oracle correlated with are the overwritten ones: the constant code's taps all see the same sum
    assert np.all(sc["oII"][1] == sc["oII"][1][:, :1]) and not np.all(sc["oII"][2] == sc["oII"][2][:, :1])


@pytest.mark.parametrize("dtype", [2, 1])
def test_full_scale_sums_come_close_to_the_bound(gc, orc, dtype):
    """The oracle's prompt sums of the full-scale scene, before the 1/32 scale: above 0.98 of 262144 x 128 x 32 for the
    channel at phase 0 (one sample in a hundred is -127 whatever the chip: half of those count against the sum), and
    for IQ samples above 0.98 of 262144 x 255 x 23 at 4.5 cells, 0.97 of the bound."""
    sc = pe.full_scale_scene(gc, orc, dtype)
    assert np.all(sc["ons"][:2] == pe.NSAMP_MAX)
    # (the reference hands trk.QQ to the correlator as its in-phase output, ref src/sdrtrk.c:42)
    big = np.abs(sc["oQQ"][:, :, 0]) * 32.0
    assert big[0].min() > 0.98 * pe.NSAMP_MAX * 128 * 32
    if dtype == 2:
        assert big[1].min() > 0.98 * pe.NSAMP_MAX * 255 * 23
        assert big[1].min() > 0.97 * pe.accumulator_bound(*pe.header_lut())
    assert max(np.abs(sc["oII"]).max(), np.abs(sc["oQQ"]).max()) * 32.0 < 2 ** 31


@pytest.mark.parametrize("dtype", [1, 2])
def test_mixed_lengths_share_no_geometry(gc, orc, dtype):
    for swapped in (False, True):
        short, long_ = pe.mixed_scenes(gc, orc, dtype, swapped)
        assert {short["ftype"], long_["ftype"]} == {1, 2} and (short["ftype"] == 2) == swapped
        assert short["ons"].max() <= pe.SHORT_NSAMP + 1 and long_["ons"][:, 1:].min() >= pe.NSAMP_MAX - 1


# ---- acquisition scenes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pe.PLAIN_SCEN)
def test_acquisition_scenarios_are_decided_where_they_were_placed(gc, orc, synth, name):
    """Every scenario: the satellites at lag 0, nsamp - 1 and nsamp - 2 nsampchip at their lags and bins, the acquired
    ones with a peak ratio of at least 1.5 ACQTH -- element 0 keeps the one at lag 0, and from two samples per chip on
    the one at lag nsamp - 1, from being acquired at any C/N0 (period_edge_cases) -- and every decision
    acq_cases.MARGIN from a tie; the absent PRN fails."""
    sc = pe.acq_scene(gc, orc, synth, name)
    pe.check_intended(sc)
    for (c, _), w in zip(sc["pairs"], sc["wants"]):
        ac.check_margins(w, (name, c.prn))
        print(f"{name} prn {c.prn}: acq {w['flagacq']} iters {w['iters']} lag {w['acqcodei']} bin {w['freqi']} "
              f"peakr {w['peakr']:.2f} cn0 {w['cn0']:.1f}")
    assert (sc["n"] > pe.ACQ_LH) == (name in ("iq16385", "iq32768", "real32768")) and sc["n"] <= pe.ACQ_L


@pytest.mark.parametrize("name", pe.COH_SCEN)
def test_coherent_scenarios(gc, orc, synth, name):
    sc = pe.coh_scene(gc, orc, synth, name)
    pe.check_intended(sc)
    for (c, _), w in zip(sc["pairs"], sc["wants"]):
        ac.check_margins(w, (name, c.prn))
        assert w["ncoh"] == 2 and w["iters"] in (2, 4)


def test_refinement_at_32768_is_decided_with_room(gc, orc, synth):
    """nref 2 on the 32768-sample IQ scenario: q* leads every other q by more than acq_fine_cases.GAP, the satellite 37
    Hz off its bin lands within 1/(4 nref ctime) of its frequency, and the prompt sums -- of the longest period a
    search takes -- fit 2^28."""
    sc = pe.acq_scene(gc, orc, synth, "iq32768")
    fine = fc.fine_all(orc, sc["pairs"], sc["W"], len(sc["W"]), sc["wants"], 2)
    assert [f["nref"] for f in fine] == [0, 0, 2, 0]            # (the acquired channel: period_edge_cases)
    f, d = fine[2], pe.ACQ_DOP[2]
    print(f"iq32768 nref 2: q {f['q']} fine {f['finefreq']:.2f} Hz (satellite at {d} Hz) quality {f['quality']:.3f} "
          f"gap {f['gap']:.3g} largest prompt sum {np.abs(f['prompt']).max()}")
    assert f["gap"] > fc.GAP and abs(f["finefreq"] - d) <= 1.0 / (4.0 * 2 * 1e-3)
    assert 1 << 19 < np.abs(f["prompt"]).max() < 1 << 28
