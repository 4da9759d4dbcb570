"""A context that is reconfigured while it lives (-m gpu): a receiver keeps one context for hours, calls
gnsscorr_set_channels again when the satellite list changes, re-creates a ring when a front end is switched, and turns
coherent integration, bit-edge hypotheses, refinement, the schedule and the lock monitor on and off.

The bar everywhere: a *live* engine that ran configuration A, had its results fetched and was reconfigured to B gives,
for everything a caller can fetch, bit for bit what a *fresh* engine gives that only ever saw B on the same ring
contents, and what a fresh engine gives whose device buffers were all poisoned with 0xA5 (tests/reconfig_cases.py:
`same`).  No tolerances: the same kernels on the same inputs, any difference is state carried over.  One scenario per
subsystem also holds the fresh engine against the oracle with the bars of tests/test_gpu_acq.py, test_gpu_tracking.py
and test_gpu_loop.py (decisions, sums and remainders exact; peakr and cn0 to 1e-4; the loop filters' atan to 1e-14 from
identical inputs), and every comparison asserts that A and B give different bytes and that the searched satellites are
acquired.  tests/test_reconfig_host.py shows on the oracle alone that every search here is decided with margin.

gnsscorr_create needs a device, so every refusal that depends on a context's state is here and not in the host file.
The refusal tests of gnsscorr_ring_create launch nothing against a mismatched ring: the call is refused before anything
is touched, and all their device work runs on the intact configuration."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import acq_fine_cases as fc
import reconfig_cases as rc

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
N4 = rc.N4
SPAN4 = 11 * N4                         # iq4's and real4's search span: the search of every 4.092 Msps test ends here


@contextlib.contextmanager
def engines(gc, k=3, poisoned=(2,)):
    """k engines, those at `poisoned` with every device buffer they will allocate poisoned; by default (live, fresh,
    poisoned fresh)."""
    es = [gc.Engine(0) for _ in range(k)]
    for i in poisoned:
        es[i].debug_poison(rc.POISON)
    try:
        yield es
    finally:
        for e in es:
            e.close()


def _code(gc, call, *args):
    """Return code and message of a C entry point called directly."""
    return call(*args), gc.lib().gnsscorr_last_error().decode()


def _refused(gc, fn, code_word):
    with pytest.raises(gc.GnsscorrError, match=code_word):
        fn()


def _schedule_is_off(gc, eng):
    """The five calls of a schedule that is off: GNSSCORR_ESTATE, each naming itself."""
    L, h = gc.lib(), eng.h
    nch = len(eng.channels)
    st = (gc.RxStat * nch)()
    prm = gc.LockPrm(**rc.RX_PRM)
    for name, rcode in (("rx_step", L.gnsscorr_rx_step(h, rc.RX_STEP)), ("rx_set", L.gnsscorr_rx_set(h, 0, gc.CH_IDLE)),
                        ("rx_status", L.gnsscorr_rx_status(h, st)), ("rx_lock_set", L.gnsscorr_rx_lock_set(h, 0, nch, C.byref(prm))),
                        ("rx_lock_status", L.gnsscorr_rx_lock_status(h, None, None))):
        assert rcode == ESTATE, (name, rcode)


# ---- 1. shrink -------------------------------------------------------------------------------------------------------
def test_shrunk_channel_set_matches_fresh_engines(gc, orc, synth):
    """Six channels with 13 taps -> two channels with 3 taps: batches (the repeated length on the look-ahead plan), the
    closed loop in chunks (1, 59) and a search with refinement, every buffer of the smaller set living inside what the
    larger one left behind."""
    s, ringlen = rc.stream(gc, orc, synth, "iq4", rc.TRK_PERIODS)
    A, B = rc.iq4_set(gc, rc.IQ4_SIX_A, 6), rc.iq4_set(gc, rc.IQ4_TWO_B, 1, nref=2)
    keep = {}

    def run_b(e):
        e.set_channels(B)
        keep["loops"], keep["starts"] = rc.loop_states(e), rc.start_states(e)
        return dict(batches=rc.obs_batches(e, rc.trk_states(B, 21), (12, 12, 30)),
                    loop=rc.obs_loop(e, (1, 59), keep["starts"], keep["loops"]), search=rc.obs_search(e, SPAN4, power_ch=1))

    with engines(gc) as (live, fresh, poisoned):
        for e in (live, fresh, poisoned):
            rc.load(e, 2, s, ringlen)
        live.set_channels(A)
        a = dict(batches=rc.obs_batches(live, rc.trk_states(A, 22), (12, 12, 30)),
                 loop=rc.obs_loop(live, (40,), rc.start_states(live), rc.loop_states(live)), search=rc.obs_search(live, SPAN4))
        got = [run_b(e) for e in (live, fresh, poisoned)]
    rc.same(got[0], got[1], "live vs fresh")
    rc.same(got[0], got[2], "live vs poisoned fresh")
    # the yardstick against the oracle: search, open-loop batches, closed loop
    b = got[1]
    assert rc.acquired(b["search"]["res"]) == [1, 1] and rc.acquired(a["search"]["res"]) == [1, 1, 1, 1, 0, 0]
    rc.check_search(b["search"]["res"], B, rc.wants(gc, orc, synth, "iq4"), "shrink")
    assert [f["nref"] for f in b["search"]["fine"][0]] == [2, 2] and b["search"]["fine"][1][:, :2].any()
    rc.anchor_batches(orc, B, s, ringlen, rc.trk_states(B, 21), b["batches"], 3)
    rc.anchor_loop(orc, B, s, ringlen, keep["starts"], keep["loops"], b["loop"])
    # A and B are different work: channel 0 is another satellite with other taps
    rc.differ(a["search"]["res"][0], b["search"]["res"][0])
    rc.differ(a["batches"]["batches"][0][0][0, :, :3], b["batches"]["batches"][0][0][0])
    rc.differ(a["loop"]["state"][0], b["loop"]["state"][0])


# ---- 2. grow, on the paths tests/test_gpu_lifecycle.py leaves out ------------------------------------------------------
def test_grown_channel_set_searches_and_tracks_closed_loop_like_fresh_engines(gc, orc, synth):
    """Two channels -> six channels with more taps: the search, the device hand-over of the acquired channels into the
    closed loop, and the closed loop of all six."""
    s, ringlen = rc.stream(gc, orc, synth, "iq4", rc.TRK_PERIODS)
    A, B = rc.iq4_set(gc, rc.IQ4_TWO_A, 2), rc.iq4_set(gc, rc.IQ4_SIX_B, 3)

    def run_b(e):
        e.set_channels(B)
        e.trk_set_state(rc.start_states(e))
        e.loop_set(rc.loop_states(e))
        out = dict(search=rc.obs_search(e, SPAN4, power_ch=3))
        e.loop_start_from_acq()
        out["loop"] = rc.obs_loop(e, (40,))
        return out

    with engines(gc) as (live, fresh, poisoned):
        for e in (live, fresh, poisoned):
            rc.load(e, 2, s, ringlen)
        live.set_channels(A)
        a = dict(batches=rc.obs_batches(live, rc.trk_states(A, 23), (12,)),
                 loop=rc.obs_loop(live, (10,), rc.start_states(live), rc.loop_states(live)), search=rc.obs_search(live, SPAN4))
        got = [run_b(e) for e in (live, fresh, poisoned)]
    rc.same(got[0], got[1], "live vs fresh")
    rc.same(got[0], got[2], "live vs poisoned fresh")
    b = got[1]
    assert rc.acquired(b["search"]["res"]) == [1, 1, 0, 1, 1, 0] and rc.acquired(a["search"]["res"]) == [1, 1]
    rc.check_search(b["search"]["res"], B, rc.wants(gc, orc, synth, "iq4"), "grow")
    # the hand-over reached the loop: an acquired channel starts at the search's buffloc with cnt 0 and ran all periods
    log, ndone = b["loop"]["chunks"][0][3:5]
    assert list(ndone) == [40] * 6 and log["buffloc"][0, 0] == b["search"]["res"][0]["buffloc"]
    assert b["loop"]["loop"][0].cnt == 40 and b["loop"]["loop"][2].cnt == 2001 + 7 * 2 + 40
    rc.differ(a["search"]["res"][0], b["search"]["res"][0])
    rc.differ(a["loop"]["state"][0], b["loop"]["state"][0])


# ---- 3. transform length both ways ------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,then", [("m26", "iq4"), ("iq4", "m26")])
def test_transform_length_changes_both_ways(gc, orc, synth, first, then):
    """32768 <-> 65536 points on one context, the ring re-created with another length under the old channels first
    (legal: the same dtype, longer than their period).  Results, one power array, the refinement with nref 2 and a
    batch; gnsscorr_acq_set_bitedge is accepted on the 32768-point set and refused on the 65536-point one."""
    sa, ringlen_a = rc.stream(gc, orc, synth, first, 20 if first == "iq4" else None)
    sb, ringlen_b = rc.stream(gc, orc, synth, then, 20 if then == "iq4" else None)
    A, B = rc.scen_set(gc, first, 2, nref=2), rc.scen_set(gc, then, 2, nref=2)
    wa, wb = len(fc.scenario(gc, orc, synth, first)[0]), len(fc.scenario(gc, orc, synth, then)[0])
    assert ringlen_a != ringlen_b and max(c.nsamp for c in A) + 116 <= ringlen_b

    def run_b(e):
        e.set_channels(B)
        out = dict(search=rc.obs_search(e, wb), batches=rc.obs_batches(e, rc.trk_states(B, 31), (3,)))
        n = len(B)
        if then == "m26":
            _refused(gc, lambda: e.acq_set_bitedge([0] * n), "65536-point")
        else:
            e.acq_set_coherent([10] * n)
            e.acq_set_bitedge([1] * n)
            assert e.acq_get_bitedge() == [1] * n
        return out

    with engines(gc) as (live, fresh, poisoned):
        rc.load(live, 2, sa, ringlen_a)
        live.set_channels(A)
        a = dict(search=rc.obs_search(live, wa), batches=rc.obs_batches(live, rc.trk_states(A, 32), (3,)))
        rc.load(live, 2, sb, ringlen_b)                 # under the old channels
        for e in (fresh, poisoned):
            rc.load(e, 2, sb, ringlen_b)
        got = [run_b(e) for e in (live, fresh, poisoned)]
    rc.same(got[0], got[1], "live vs fresh")
    rc.same(got[0], got[2], "live vs poisoned fresh")
    b = got[1]
    want = rc.wants(gc, orc, synth, then)
    assert rc.acquired(b["search"]["res"]) == [int(c.prn in rc.present(then)) for c in B]
    assert rc.acquired(a["search"]["res"]) == [int(c.prn in rc.present(first)) for c in A]
    rc.check_search(b["search"]["res"], B, want, then)
    assert b["search"]["fine"][0][0]["nref"] == 2 and b["search"]["power"].shape == (B[0].nfreq, B[0].nsamp)
    rc.differ(a["search"]["res"][0], b["search"]["res"][0])


# ---- 4. acquisition settings do not survive set_channels --------------------------------------------------------------
def test_acquisition_settings_do_not_survive_set_channels(gc, orc, synth):
    """`coh` with ncoh 10, every bit-edge hypothesis and nref 10; then gnsscorr_set_channels itself (the C entry point,
    which does not re-apply the settings as Engine.set_channels does) with the very same descriptors: the getters read
    1 / 0 / 0 and the search is a fresh plain one.  Settings applied after it give coh's own fresh results."""
    s, ringlen = rc.stream(gc, orc, synth, "coh")
    coh, plain = rc.scen_set(gc, "coh", 2, nref=10), rc.scen_set(gc, "coh", 2, plain=True)
    n = len(coh)
    assert [(c.ncoh, c.estep, c.nref) for c in coh] == [(10, 1, 10)] * n and [(c.ncoh, c.estep, c.nref) for c in plain] == [(1, 0, 0)] * n
    with engines(gc, 5, poisoned=(2, 4)) as (live, fresh_plain, poisoned_plain, fresh_coh, poisoned_coh):
        for e in (live, fresh_plain, poisoned_plain, fresh_coh, poisoned_coh):
            rc.load(e, 2, s, ringlen)
        live.set_channels(coh)
        assert (live.acq_get_coherent(), live.acq_get_bitedge(), live.acq_get_refine()) == ([10] * n, [1] * n, [10] * n)
        a = rc.obs_search(live, len(s))
        arr = (gc.ChanDesc * n)(*[c.desc() for c in coh])
        assert gc.lib().gnsscorr_set_channels(live.h, n, arr) == 0
        assert (live.acq_get_coherent(), live.acq_get_bitedge(), live.acq_get_refine()) == ([1] * n, [0] * n, [0] * n)
        _refused(gc, live.acq_fetch, "no acq_run yet")              # the last search's results went with the old set
        p_live = rc.obs_search(live, len(s))
        p = []
        for e in (fresh_plain, poisoned_plain):
            e.set_channels(plain)
            p.append(rc.obs_search(e, len(s)))
        # conversely: the settings, applied after the second set_channels
        live.acq_set_coherent([10] * n)
        live.acq_set_bitedge([1] * n)
        live.acq_set_refine([10] * n)
        c_live = rc.obs_search(live, len(s))
        c = []
        for e in (fresh_coh, poisoned_coh):
            e.set_channels(coh)
            c.append(rc.obs_search(e, len(s)))
    for k in (0, 1):
        rc.same(p_live, p[k], ("plain", k))
        rc.same(c_live, c[k], ("coh", k))
    rc.same(a, c[0], "the first search was coh's own")
    # plain: every edge -1, the refinement is rule 8
    assert p[0]["edge"] == [-1] * n and not p[0]["fine"][1].any()
    assert p[0]["fine"][0] == [dict(finefreq=r["acqfreq"], quality=0.0, q=0, nref=0) for r in p[0]["res"]]
    rc.check_search(p[0]["res"], plain, rc.wants(gc, orc, synth, "coh", plain=True), "plain")
    want = rc.wants(gc, orc, synth, "coh")
    rc.check_search(c[0]["res"], coh, want, "coh")
    assert c[0]["edge"] == [want[ch.prn]["edge"] for ch in coh] and min(c[0]["edge"]) > 0
    assert [f["nref"] for f in c[0]["fine"][0]] == [10] * n and rc.acquired(p[0]["res"]) == rc.acquired(c[0]["res"]) == [1] * n
    rc.differ(p[0]["res"], c[0]["res"])
    rc.differ(p[0]["power"], c[0]["power"])


# ---- 5. schedule and lock monitor --------------------------------------------------------------------------------------
def _rx_load(gc, eng, prns, corrn, sig, wrpos):
    eng.ring_create(1, 2, rc.RX_RING)
    rc.rx_feed(eng, sig, wrpos)
    eng.set_channels(rc.rx_chans(gc, prns, corrn))


def _check_rx_against_oracle(gc, orc, synth, steps, prns, wrpos_list):
    """The yardstick of the schedule tests: every search a step reports is the restated one at that write position, and
    the walk is the one the scenario was built for."""
    want = rc.rx_wants(gc, orc, synth)
    chans = rc.rx_chans(gc, prns, 2)
    searched = 0
    for k, (o, wp) in enumerate(zip(steps, wrpos_list)):
        for c, st in zip(chans, o["status"]):
            if st["acq_wrpos"] == wp and st["attempts"]:
                rc.check_search([st["acq"]], [c], want[wp], ("rx", k))
                searched += 1
    return searched


def test_set_channels_under_a_running_schedule_with_a_monitor_launch_pending(gc, orc, synth):
    sig = rc.rx_signal(gc, synth)
    steps_b = rc.RX_WRPOS[:3]
    with engines(gc) as (live, fresh, poisoned):
        _rx_load(gc, live, rc.RX_A, 2, sig, 0)
        rc.rx_begin(live)
        a = rc.rx_steps(live, sig, rc.RX_A_WRPOS[:1])
        assert [st["state"] for st in a[0]["status"]] == [gc.CH_TRACK, gc.CH_TRACK, gc.CH_SEARCH]
        rc.rx_feed(live, sig, rc.RX_A_WRPOS[1])
        live.rx_step(rc.RX_STEP)                        # its monitor launch is pending: nothing is fetched or waited for
        live.set_channels(rc.rx_chans(gc, rc.RX_B, 3))
        _schedule_is_off(gc, live)
        for e in (fresh, poisoned):
            _rx_load(gc, e, rc.RX_B, 3, sig, steps_b[0])
            _schedule_is_off(gc, e)
        got = []
        for e in (live, fresh, poisoned):
            rc.rx_begin(e)
            got.append(rc.rx_steps(e, sig, steps_b))
    rc.same(got[0], got[1], "live vs fresh")
    rc.same(got[0], got[2], "live vs poisoned fresh")
    b = got[1]
    assert _check_rx_against_oracle(gc, orc, synth, b, rc.RX_B, steps_b) >= 6
    # the walk: both satellites acquired in the first step, declared lost in the second (rule 1: no bit synchronisation
    # 15 periods after the hand-over), searched and acquired again in the third; the absent PRN searched every step
    T, S = gc.CH_TRACK, gc.CH_SEARCH
    assert [[st["state"] for st in o["status"]] for o in b] == [[T, S, T]] * 3
    assert [list(o["losses"]) for o in b] == [[0, 0, 0], [0, 0, 0], [1, 0, 1]]
    assert [st["attempts"] for st in b[2]["status"]] == [2, 3, 2]
    assert b[1]["lock"]["lost"][0] == 1 and b[1]["lock"]["reason"][0] == 1 and b[1]["lock"]["lost_cnt"][0] == rc.RX_PRM["sync_periods"] - 1
    assert b[2]["lock"]["lost"][0] == 0 and b[2]["status"][0]["cnt"] == b[2]["log"][1][0] > 0      # cnt restarted
    assert all(o["log"][1][1] == 0 and not o["trk"][0][1].any() for o in b)                        # SEARCH: no period
    rc.differ(a[0]["status"][0], b[0]["status"][0])


def test_rx_start_again_on_the_same_channels(gc, orc, synth):
    """gnsscorr_rx_start a second time, no gnsscorr_set_channels between, after the ring has moved on, against a fresh
    engine fed to the same write position.  The schedule starts over; the device's loop states survive the call, which
    shows in rx_status's cnt until the next hand-over (the header says so) and nowhere after it."""
    sig = rc.rx_signal(gc, synth)
    with engines(gc) as (live, fresh, poisoned):
        _rx_load(gc, live, rc.RX_B, 3, sig, 0)
        rc.rx_begin(live)
        a = rc.rx_steps(live, sig, rc.RX_WRPOS[:2])
        cnt = [st["cnt"] for st in a[1]["status"]]
        assert cnt[0] > 0 and cnt[2] > 0 and cnt[1] == 0
        rc.rx_feed(live, sig, rc.RX_WRPOS[3])
        for e in (fresh, poisoned):
            _rx_load(gc, e, rc.RX_B, 3, sig, rc.RX_WRPOS[3])
        live.rx_start(rc.RX_RETRY_MS)                   # the loop constants are still set: no loop_set needed
        st = live.rx_status()
        assert [s["state"] for s in st] == [gc.CH_SEARCH] * 3 and [s["attempts"] for s in st] == [0] * 3
        assert [s["cnt"] for s in st] == cnt            # the finding, pinned: the device's count survives rx_start
        lock, losses = live.rx_lock_status()
        assert not losses.any()
        live.rx_lock_set(rc.RX_PRM)
        got = [rc.rx_steps(live, sig, rc.RX_WRPOS[3:])]
        for e in (fresh, poisoned):
            rc.rx_begin(e)
            got.append(rc.rx_steps(e, sig, rc.RX_WRPOS[3:]))
    rc.same(got[0], got[1], "live vs fresh")
    rc.same(got[0], got[2], "live vs poisoned fresh")
    b = got[1]
    assert _check_rx_against_oracle(gc, orc, synth, b, rc.RX_B, rc.RX_WRPOS[3:]) == 3
    assert [s["state"] for s in b[0]["status"]] == [gc.CH_TRACK, gc.CH_SEARCH, gc.CH_TRACK]
    assert b[0]["status"][0]["cnt"] == b[0]["log"][1][0] > 0
    rc.differ(a[1]["status"][0], b[0]["status"][0])


# ---- 6. ring re-create under live channels -----------------------------------------------------------------------------
def _variant_stream(gc, orc, synth, name, periods, seed):
    """The scenario's span with other noise behind it: another ring content for every re-create."""
    sc = fc.SCEN[name]
    W = fc.scenario(gc, orc, synth, name)[0]
    s = np.concatenate([W, rc.ac.noise(periods * N4 - len(W), sc["dtype"], seed)])
    return s, rc.ec.granule(len(s), sc["dtype"])


@pytest.mark.parametrize("name", ["iq4", "real4"])
def test_ring_recreated_with_the_same_dtype_under_live_channels(gc, orc, synth, name):
    """Another length, owned -> caller-owned memory -> owned: the write position reads 0, a search before the samples
    are back is refused, the channels' states, the loop states and the last search's results stay, and after a push and
    trk_set_state a batch, a closed loop and a search equal fresh engines'."""
    dtype = fc.SCEN[name]["dtype"]
    S = rc.scen_set(gc, name, 2, nref=2)
    n = len(S)
    variants = [(60, 7001, False), (rc.TRK_PERIODS, 7002, True), (48, 7003, False)]     # periods, noise seed, devmem
    keep = {}

    def observe(e, s):
        e.ring_push_raw(1, s, len(s))
        keep["loops"], keep["starts"] = rc.loop_states(e), rc.start_states(e)
        return dict(batches=rc.obs_batches(e, rc.trk_states(S, 41), (12, 12)),
                    loop=rc.obs_loop(e, (20,), keep["starts"], keep["loops"]), search=rc.obs_search(e, SPAN4, power_ch=n - 1))

    s0, ringlen0 = rc.stream(gc, orc, synth, name, rc.TRK_PERIODS)
    live = gc.Engine(0)
    mem = None
    try:
        rc.load(live, dtype, s0, ringlen0)
        live.set_channels(S)
        last = dict(batches=rc.obs_batches(live, rc.trk_states(S, 42), (12,)),
                    loop=rc.obs_loop(live, (20,), rc.start_states(live), rc.loop_states(live)), search=rc.obs_search(live, SPAN4))
        for periods, seed, devmem in variants:
            s, ringlen = _variant_stream(gc, orc, synth, name, periods, seed)
            assert ringlen != ringlen0 or devmem
            held = dict(state=live.trk_get_state(), loop=live.loop_get(), res=live.acq_fetch(), fine=live.acq_fetch_fine(prompts=True))
            if devmem:
                mem = rc.DevMem(gc, dtype * ringlen)
            live.ring_create(1, dtype, ringlen, mem.p if devmem else None)
            assert live.ring_wrpos(1) == 0 and live.ring_devptr(1) is not None
            assert devmem == (mem is not None and live.ring_devptr(1) == mem.p.value)
            _refused(gc, lambda: live.acq_run(0), "holds 0 samples")
            rc.same(held, dict(state=live.trk_get_state(), loop=live.loop_get(), res=live.acq_fetch(),
                               fine=live.acq_fetch_fine(prompts=True)), "what a re-create keeps")
            got = [observe(live, s)]
            with engines(gc, 2, poisoned=(1,)) as (fresh, poisoned):
                for e in (fresh, poisoned):
                    e.ring_create(1, dtype, ringlen)
                    e.set_channels(S)
                    got.append(observe(e, s))
            rc.same(got[0], got[1], (periods, "live vs fresh"))
            rc.same(got[0], got[2], (periods, "live vs poisoned fresh"))
            b = got[1]
            assert rc.acquired(b["search"]["res"]) == [int(c.prn in rc.present(name)) for c in S]
            rc.check_search(b["search"]["res"], S, rc.wants(gc, orc, synth, name), (name, periods))
            if periods == 60:
                rc.anchor_batches(orc, S, s, ringlen, rc.trk_states(S, 41), b["batches"], 2)
                rc.anchor_loop(orc, S, s, ringlen, keep["starts"], keep["loops"], b["loop"])
            rc.differ(last["batches"]["batches"][0][0], b["batches"]["batches"][0][0], "other noise, other sums")
            last = b
    finally:
        live.close()
        if mem is not None:
            mem.free()


def test_ring_recreate_refuses_what_the_live_channels_cannot_read(gc, orc, synth):
    """dtype 2 channels on ring 1: a re-create with dtype 1, and one shorter than a code period + 100 + 16, are refused
    with GNSSCORR_EINVAL naming the channel and nothing touched -- write position, contents, and what a batch computes
    afterwards, against an engine that never saw the refused calls.  Nothing runs against a mismatched ring."""
    s, ringlen = rc.stream(gc, orc, synth, "iq4", 20)
    S = rc.iq4_set(gc, rc.IQ4_THREE, 2)
    L = gc.lib()
    with engines(gc, 2, poisoned=()) as (live, control):
        for e in (live, control):
            rc.load(e, 2, s, ringlen)
            e.set_channels(S)
        ptr = live.ring_devptr(1)
        short = N4 + 100 + 16 - 8                       # 2 * 4200 bytes: a multiple of 16, eight samples too few
        assert (2 * short) % 16 == 0 and (2 * (short + 8)) % 16 == 0
        for args, words in (((1, 1, ringlen, None), ("channel 0", "dtype 2", "dtype 1")),
                            ((1, 1, 2 * ringlen, None), ("channel 0", "dtype 1")),
                            ((1, 2, short, None), ("channel 0", "shorter than a code period"))):
            code, msg = _code(gc, L.gnsscorr_ring_create, live.h, *args)
            assert code == EINVAL and all(w in msg for w in words), (args, code, msg)
            assert live.ring_wrpos(1) == len(s) and live.ring_devptr(1) == ptr
            assert np.array_equal(live.ring_read(1, 0, len(s), 2), s)
        got = [rc.obs_batches(e, rc.trk_states(S, 51), (6, 6)) for e in (live, control)]     # the stream holds 20 periods
        rc.same(got[0], got[1], "after the refusals")
        rc.anchor_batches(orc, S, s, ringlen, rc.trk_states(S, 51), got[1], 2)
        # a ring no channel reads with another dtype, and the shortest ring the channels can read: both accepted
        live.ring_create(2, 1, 8192)
        assert live.ring_wrpos(1) == len(s) and np.array_equal(live.ring_read(1, 100, 5000, 2), s[100:5100])
        live.ring_create(1, 2, short + 8)
        assert live.ring_wrpos(1) == 0 and live.ring_devptr(1) is not None
        # once the channels are gone from the ring, its dtype may change
        live.set_channels([_on_ring2(gc)])
        live.ring_create(1, 1, ringlen)
        assert live.ring_wrpos(1) == 0


def _on_ring2(gc):
    """A real-sample channel on ring 2 (created as dtype 1 above)."""
    sc = fc.SCEN["real4"]
    c = rc.chan(gc, sc, sc["chans"][0], 2)
    c.ftype = 2
    return c


def test_ring_recreate_switches_a_running_schedule_off(gc, orc, synth):
    """The rule of include/gnsscorr.h: re-creating a ring that a channel reads switches the schedule off until the next
    gnsscorr_rx_start; a ring no channel reads leaves it alone.  After the samples are back and gnsscorr_rx_start, the
    steps are a fresh engine's."""
    sig = rc.rx_signal(gc, synth)
    steps = rc.RX_WRPOS[:2]
    with engines(gc) as (live, fresh, poisoned):
        _rx_load(gc, live, rc.RX_B, 3, sig, 0)
        rc.rx_begin(live)
        a = rc.rx_steps(live, sig, rc.RX_A_WRPOS[:1])
        live.ring_create(2, 2, 4096)                    # nobody reads ring 2
        assert [st["state"] for st in live.rx_status()] == [st["state"] for st in a[0]["status"]]
        rc.rx_feed(live, sig, rc.RX_A_WRPOS[1])
        live.rx_step(rc.RX_STEP)                        # TRACK channels, a monitor launch pending
        live.ring_create(1, 2, rc.RX_RING)
        assert live.ring_wrpos(1) == 0
        _schedule_is_off(gc, live)
        got = []
        for e in (fresh, poisoned):
            _rx_load(gc, e, rc.RX_B, 3, sig, 0)
        for e in (live, fresh, poisoned):
            rc.rx_feed(e, sig, steps[0])
            if e is live:
                e.rx_start(rc.RX_RETRY_MS)              # the channels and their loop constants stayed
                e.rx_lock_set(rc.RX_PRM)
            else:
                rc.rx_begin(e)
            got.append(rc.rx_steps(e, sig, steps))
    rc.same(got[0], got[1], "live vs fresh")
    rc.same(got[0], got[2], "live vs poisoned fresh")
    b = got[1]
    assert _check_rx_against_oracle(gc, orc, synth, b, rc.RX_B, steps) >= 4
    rc.differ(a[0]["status"][0], b[0]["status"][0])
    assert [st["state"] for st in b[1]["status"]] == [gc.CH_TRACK, gc.CH_SEARCH, gc.CH_TRACK] and b[1]["lock"]["lost"][0] == 1


# ---- 7. reconfigure while work is in flight ----------------------------------------------------------------------------
FIRST = ("trk_run", "acq_run", "trk_run_loop")
RECONF = ("set_channels", "ring_create", "acq_set_coherent")


def _in_flight_b(gc, e, reconf, s, live):
    """Reconfiguration `reconf` on engine e, whose channels are IQ4_THREE, and what B then computes.  A fresh engine
    (live False) has the ring as the live one's re-create and push leave it."""
    if reconf == "set_channels":
        B = rc.iq4_set(gc, rc.IQ4_TWO_B, 1)
        e.set_channels(B)
        return dict(batches=rc.obs_batches(e, rc.trk_states(B, 61), (12, 12)), search=rc.obs_search(e, SPAN4))
    S = e.channels
    if reconf == "ring_create":
        if live:
            e.ring_create(1, 2, rc.ec.granule(len(s), 2))
            assert e.ring_wrpos(1) == 0
            e.ring_push_raw(1, s, len(s))
        return dict(batches=rc.obs_batches(e, rc.trk_states(S, 62), (12, 12)),
                    loop=rc.obs_loop(e, (20,), rc.start_states(e), rc.loop_states(e)), search=rc.obs_search(e, SPAN4))
    e.acq_set_coherent([2] * len(S))
    return dict(search=rc.obs_search(e, SPAN4), batches=rc.obs_batches(e, rc.trk_states(S, 63), (12,)))


@pytest.fixture(scope="module")
def in_flight_fresh(gc, orc, synth):
    """reconf -> [fresh, poisoned fresh] observations of B, computed once."""
    s, ringlen = rc.stream(gc, orc, synth, "iq4", rc.TRK_PERIODS)
    out = {}
    for reconf in RECONF:
        with engines(gc, 2, poisoned=(1,)) as (fresh, poisoned):
            out[reconf] = []
            for e in (fresh, poisoned):
                rc.load(e, 2, s, ringlen)
                e.set_channels(rc.iq4_set(gc, rc.IQ4_THREE, 2))
                out[reconf].append(_in_flight_b(gc, e, reconf, s, False))
    return out


@pytest.mark.parametrize("reconf", RECONF)
@pytest.mark.parametrize("first", FIRST)
def test_reconfiguration_behind_work_in_flight(gc, orc, synth, in_flight_fresh, first, reconf):
    """The quiesce paths: 30 periods of the batched tracker, a search, or 30 periods of the closed loop are queued and
    the reconfiguring call follows with no fetch or synchronisation by the caller."""
    s, ringlen = rc.stream(gc, orc, synth, "iq4", rc.TRK_PERIODS)     # holds the 60 periods queued below
    S = rc.iq4_set(gc, rc.IQ4_THREE, 2)
    live = gc.Engine(0)
    try:
        rc.load(live, 2, s, ringlen)
        live.set_channels(S)
        live.trk_set_state(rc.trk_states(S, 64))
        live.loop_set(rc.loop_states(live))
        if first == "trk_run":
            live.trk_run(30)
            live.trk_run(30)                            # the second on the look-ahead plan, a third being planned
        elif first == "acq_run":
            live.acq_run(SPAN4)
        else:
            live.trk_run_loop(30)
        got = _in_flight_b(gc, live, reconf, s, True)
    finally:
        live.close()
    want = in_flight_fresh[reconf]
    rc.same(got, want[0], (first, reconf, "live vs fresh"))
    rc.same(got, want[1], (first, reconf, "live vs poisoned fresh"))
    chans = rc.iq4_set(gc, rc.IQ4_TWO_B, 1) if reconf == "set_channels" else S
    assert any(rc.acquired(got["search"]["res"]))
    if reconf != "acq_set_coherent":                    # (the restated searches are those without coherent integration)
        assert rc.acquired(got["search"]["res"]) == [int(c.prn in rc.present("iq4")) for c in chans]
        rc.check_search(want[0]["search"]["res"], chans, rc.wants(gc, orc, synth, "iq4"), (first, reconf))


def test_in_flight_reconfigurations_are_different_work(in_flight_fresh):
    f = {k: v[0] for k, v in in_flight_fresh.items()}
    rc.differ(f["set_channels"]["search"]["res"][0], f["ring_create"]["search"]["res"][0])
    rc.differ(f["ring_create"]["search"]["res"], f["acq_set_coherent"]["search"]["res"])
    rc.differ(f["ring_create"]["batches"]["batches"][0][0], f["acq_set_coherent"]["batches"]["batches"][0][0])


# ---- 8. spectrum analyzer and FEC across reconfiguration ---------------------------------------------------------------
def _spectrum(e, ftype, f_sf):
    return e.spectrum(ftype, [0, 3000], 4 * 8192, f_sf, nfft=8192, nloop=8, seed=5)


def _spec_fetch_code(gc, e):
    s = np.zeros(4 * 8192)
    return _code(gc, gc.lib().gnsscorr_spec_fetch, e.h, s.ctypes.data, s.size, None, 0, None, 0, None, 0)


def test_spectrum_and_fec_across_reconfiguration(gc, orc, synth):
    """The IF monitor after a ring re-create with the other dtype (on a context without channels on that ring) and after
    set_channels, the FEC decoder after set_channels: bit for bit a fresh engine's.  set_channels drops the monitor's
    last run: gnsscorr_spec_fetch then returns GNSSCORR_ESTATE until the next gnsscorr_spec_run (the header says so)."""
    s_iq, rl_iq = rc.stream(gc, orc, synth, "iq4", 20)
    s_re, rl_re = rc.stream(gc, orc, synth, "real4", 20)
    S = rc.iq4_set(gc, rc.IQ4_THREE, 2)
    sym = np.where(np.random.default_rng(9).random((2, 200)) < 0.5, -1, 1).astype(np.int8)
    fec = lambda e: e.fec_run(sym, 43, 50, 1, win=44, ndec=16)
    with engines(gc) as (live, fresh, poisoned):
        # ring 2 holds real samples, is looked at, and is re-created as IQ; the channels live on ring 1
        rc.load(live, 2, s_iq, rl_iq)
        live.set_channels(S)
        rc.load(live, 1, s_re, rl_re, ftype=2)
        a = dict(spec=_spectrum(live, 2, rc.F4), fec=fec(live))
        rc.load(live, 2, s_iq, rl_iq, ftype=2)
        got = [dict(spec=_spectrum(live, 2, rc.F4))]
        for e in (fresh, poisoned):
            rc.load(e, 2, s_iq, rl_iq, ftype=2)
            got.append(dict(spec=_spectrum(e, 2, rc.F4)))
        rc.same(got[0], got[1], "spectrum after a re-create with the other dtype, vs fresh")
        rc.same(got[0], got[2], "vs poisoned fresh")
        assert got[1]["spec"][3][:, 1].any() and not a["spec"][3][:, 1].any()      # Q histogram: IQ now, real before
        assert a["spec"][1].shape != got[1]["spec"][1].shape
        # set_channels: the last run is gone, the next one and the decoder are a fresh engine's
        assert _spec_fetch_code(gc, live)[0] == 0
        live.set_channels(rc.iq4_set(gc, rc.IQ4_TWO_B, 1))
        code, msg = _spec_fetch_code(gc, live)
        assert code == ESTATE and "no spec_run yet" in msg
        after = [dict(spec=_spectrum(live, 2, rc.F4), fec=fec(live))]
        for e in (fresh, poisoned):
            rc.load(e, 2, s_iq, rl_iq)
            e.set_channels(rc.iq4_set(gc, rc.IQ4_TWO_B, 1))
            after.append(dict(spec=_spectrum(e, 2, rc.F4), fec=fec(e)))
        rc.same(after[0], after[1], "after set_channels, vs fresh")
        rc.same(after[0], after[2], "vs poisoned fresh")
        rc.same(after[0]["spec"], got[0]["spec"], "the same ring, the same spectrum")
        rc.same(after[0]["fec"], a["fec"], "the decoder depends on no channel set")
        assert after[1]["fec"].any() and after[1]["spec"][2].any()
