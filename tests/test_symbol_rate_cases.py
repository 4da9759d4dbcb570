"""CPU checks of tests/symbol_rate_cases.py: on the oracle alone, every scenario tests/test_gpu_symbols_rates.py runs is
what it claims -- the oracle has the samples for every period (flagtrk 1), the lengths have the segment counts they
are named for, the boundary channel's periods fall on both sides of the boundary, every satellite of the acquisition
scenarios is acquired in the first window with a peak ratio of 1.5 ACQTH or more (period_edge_cases.check_intended's
margin: a condition on the inputs, not on the library), and the absent PRN fails."""
import pytest

import acq_cases as ac
import period_edge_cases as pe
import symbol_cases as sc
import symbol_rate_cases as rc


@pytest.mark.parametrize("ring", (1, 2))
def test_sequence_lengths_and_segments(orc, ring):
    """A.1 / A.4: the queue's segment counts grow three times, then fall back to one; every period has its samples."""
    chans = rc.seq(ring)
    assert [pe.nseg(ring, c["nsamp"]) for c in chans] == rc.SEQ_NSEG
    assert [rc.queue_nseg(ring, c["nsamp"]) for c in chans] == rc.SEQ_QUEUE_NSEG
    assert pe.nseg(ring, pe.first_nsamp(ring, 3) - 1) == 2
    assert rc.periods(pe.NSAMP_MAX, rc.SEQ_CAP) == 2 and rc.periods(65536, rc.SEQ_CAP) == rc.SEQ_CAP
    for c in chans:
        rows = rc.oracle_rows(orc, c, rc.periods(c["nsamp"], rc.SEQ_CAP))
        assert all(abs(r[0][0] - c["nsamp"]) <= 100 for r in rows), c["key"]
    assert [c["key"] for c in rc.after(ring)] == [chans[3]["key"], chans[4]["key"]]
    assert [c["nsamp"] for c in rc.after(ring)] == [pe.NSAMP_MAX, 2048]


@pytest.mark.parametrize("which", rc.BOUNDARIES)
@pytest.mark.parametrize("ring", (1, 2))
def test_boundary_periods_fall_on_both_sides(orc, ring, which):
    """A.2: consecutive currnsamp of n - 1 and n, where n = first_nsamp(dtype, 2) is the first length an engine gives two
    segments ("engine") and n = first_nsamp + 100 the first the queue launches with two ("queue")."""
    c = rc.boundary(ring, which)
    first = pe.first_nsamp(ring, 2)
    assert (pe.nseg(ring, first - 1), pe.nseg(ring, first)) == (1, 2)
    n = c["nsamp"]
    assert n == first + (100 if which == "queue" else 0)
    if which == "queue":
        assert (rc.queue_nseg(ring, n - 1), rc.queue_nseg(ring, n)) == (1, 2)
    rows = rc.oracle_rows(orc, c, rc.BOUNDARY_NPER, state=rc.BOUNDARY_STATE[ring])
    ns = [r[0][0] for r in rows]
    print(f"\nring {ring} {which}: nsamp {n}, currnsamp {ns}")
    assert len(ns) == 6 and set(ns) == {n - 1, n}, ns
    assert sum(a != b for a, b in zip(ns, ns[1:])) >= 3, ns


@pytest.mark.parametrize("ring", (1, 2))
def test_mixed_groups(orc, ring):
    """A.3: two groups per ring; the corrn 2 group holds every length under tap sets of smax 6 and 16; the short members
    track on after the longest have finished; no more than 55 requests at a time."""
    chans = rc.mixed(ring)
    groups = {}
    for c in chans:
        groups.setdefault(sc.TAPS[c["taps"]][0], []).append(c)
    assert sorted(groups) == [2, 6]
    assert sorted({c["nsamp"] for c in groups[2]}) == [2048, 16368, pe.first_nsamp(ring, 3), pe.NSAMP_MAX]
    for n in {c["nsamp"] for c in groups[2]}:
        assert {c["taps"] for c in groups[2] if c["nsamp"] == n} == {"A", "B"}
    assert {rc.queue_nseg(ring, c["nsamp"]) for c in groups[2]} == {1, 2, 11}
    assert {rc.queue_nseg(ring, c["nsamp"]) for c in groups[6]} == {1, 3}
    assert len(rc.mixed(1)) + len(rc.mixed(2)) <= 55
    for c in chans:
        nper = rc.mixed_nper(c)
        assert nper >= 2 and (nper == 2) == (c["nsamp"] == pe.NSAMP_MAX), (c["key"], nper)
        rc.oracle_rows(orc, c, nper)
    assert rc.mixed_nper(groups[2][0]) == rc.MIXED_CAP
    for k in range(rc.PAIR_TRIES):
        b, s, l = rc.pair(ring, k)
        assert sc.TAPS[b["taps"]][0] != sc.TAPS[s["taps"]][0] == sc.TAPS[l["taps"]][0]
        assert (s["nsamp"], l["nsamp"]) == (2048, pe.NSAMP_MAX)
        for c in (b, s, l):
            rc.oracle_rows(orc, c, 1, salt=k)


@pytest.mark.parametrize("name", list(rc.RATES))
def test_rate_satellite_is_acquired_in_the_first_window(gc, orc, synth, name):
    """B: nsamp and the transform each rate names; the oracle acquires in its first window with room, every decision of
    that window acq_cases.MARGIN from a tie; the six periods behind the hand-over have their samples and hold the
    satellite."""
    r = rc.RATES[name]
    buf = rc.acq_recording(gc, synth, name)
    o, w = rc.oracle_search(orc, name, buf)
    assert o.nsampchip == r["nsamp"] // 1023
    assert (r["nsamp"] > pe.ACQ_LH) == (name in ("fft64k_16385", "longest_32768")) and r["nsamp"] <= pe.ACQ_L
    print(f"\n{name}: flagacq {w['flagacq']} iteration {w['iters']} codei {w['acqcodei']} freqi {w['freqi']} peakr {w['peakr']:.2f} "
          f"cn0 {w['cn0']:.1f}")
    assert w["flagacq"] == 1 and w["iters"] == 1 and w["peakr"] >= 1.5 * 3.0, (name, w["flagacq"], w["iters"], w["peakr"])
    assert abs(w["acqfreq"] - r["f_if"] - r["doppler"]) <= 100.0
    assert 2 * o.nsampchip < w["acqcodei"] < r["nsamp"] - 2 * o.nsampchip - 1
    c = rc.acq_chan(name)
    steps = ac.oracle_acq(orc, rc.cut_grid(sc.oracle_chan(orc, c), c), buf, sc.RINGLEN, len(buf))
    assert (steps["flagacq"], steps["iters"], steps["peakr"]) == (1, 1, w["peakr"])
    ac.check_margins(steps, name)
    rows, _ = sc.oracle_track(orc, o, orc.make_ring(buf, sc.RINGLEN, len(buf)), w["buffloc"], rc.ACQ_NPER)
    ip = sc.prompt_power(rows)
    print(f"{name}: min prompt power {min(ip) / rc.power_floor(r['nsamp']):.1f} x the floor")
    assert min(ip) > rc.power_floor(r["nsamp"])


def test_absent_prn_fails_on_the_oracle(gc, orc, synth):
    name, prn = rc.ABSENT
    assert prn != rc.RATES[name]["prn"]
    _, w = rc.oracle_search(orc, name, rc.acq_recording(gc, synth, name), prn=prn)
    assert w["flagacq"] == 0 and w["iters"] == rc.ACQ_INTG and w["peakr"] < 3.0 * (1 - ac.MARGIN)
    c = rc.acq_chan(name, prn)
    buf = rc.acq_recording(gc, synth, name)
    ac.check_margins(ac.oracle_acq(orc, rc.cut_grid(sc.oracle_chan(orc, c), c), buf, sc.RINGLEN, len(buf)), "absent PRN")


def test_reinit_last_search_is_decided_with_room(gc, orc, synth):
    """The re-initialised struct's last search: 2048-sample windows over the 16.384 Msps recording, which holds nothing
    at that rate.  Whatever the oracle finds in each window, it finds acq_cases.MARGIN away from a tie."""
    na, nb = rc.REINIT
    buf = rc.acq_recording(gc, synth, na)
    c = rc.acq_chan(nb)
    w = ac.oracle_acq(orc, rc.cut_grid(sc.oracle_chan(orc, c), c), buf, sc.RINGLEN, len(buf))
    ac.check_margins(w, "2048-sample search of the 16.384 Msps recording")
    full = rc.oracle_search(orc, nb, buf)[1]
    print(f"\nflagacq {w['flagacq']} at iteration {w['iters']}, peakr {w['peakr']:.3f}")
    assert (full["flagacq"], full["iters"], full["buffloc"], full["peakr"]) == (w["flagacq"], w["iters"], w["buffloc"], w["peakr"])
    found = rc.oracle_search(orc, na, buf)[1]
    assert (found["acqcodei"], found["buffloc"]) != (full["acqcodei"], full["buffloc"])     # (the old engine's answer is another)


def test_refused_rate_and_reinit_rates(orc):
    """The 65.536 Msps struct lies above the search's limit and tracks on the tracking rings; the re-initialised struct
    changes rate on one ring (same sample type: the ring comes back with the same length)."""
    assert rc.REFUSED_NSAMP > pe.ACQ_L and (rc.ACQ_INTG + 1) * rc.REFUSED_NSAMP < rc.WRPOS
    c = rc.rate_chan("refused", 2, "A", 21, rc.REFUSED_NSAMP)
    assert sc.oracle_chan(orc, c).nsamp == rc.REFUSED_NSAMP
    b0 = rc.WRPOS - (rc.ACQ_INTG + 1) * rc.REFUSED_NSAMP
    assert b0 + (rc.REFUSED_NPER + 1) * (rc.REFUSED_NSAMP + 100) < rc.WRPOS
    o = sc.oracle_chan(orc, c)
    sc.hand_over(o, rc.start(c)[0], o.crate)
    rows, _ = sc.oracle_track(orc, o, orc.make_ring(rc.ring_samples()[1], sc.RINGLEN, rc.WRPOS), b0, rc.REFUSED_NPER)
    assert len(rows) == rc.REFUSED_NPER and rc.queue_nseg(2, rc.REFUSED_NSAMP) == 3
    a, b = (rc.RATES[k] for k in rc.REINIT)
    assert a["dtype"] == b["dtype"] and a["nsamp"] != b["nsamp"]
