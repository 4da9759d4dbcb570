"""The mixed-receiver scenarios of tests/rx_mixed_cases.py on the CPU oracle alone (no GPU): they decide what
tests/test_gpu_rx_mixed.py relies on.  Present channels are acquired at the attempt claimed, absent ones fail every
attempt, late ones fail first and are acquired then; every search -- failed ones included, at every iteration up
to the deciding one -- stands acq_cases.MARGIN from a tie between lags, a tie between Doppler rows and the
threshold.  Conditions on the inputs (seeds, C/N0, switch-on times), not tolerances.  Also: synth.make_if's
optional per-satellite t_off, held to the byte identities t_on is held to in tests/test_rx_host.py."""
import ctypes as C
import hashlib

import numpy as np

import acq_cases as ac
import rx_mixed_cases as mc


def test_mix_schedule_is_what_the_scenario_claims():
    wps = mc.mix_wrpos()
    assert len(wps) == mc.NSTEP and wps[0] == (6 * mc.N1, 0) and wps[2][1] == 0 and wps[3][1] == mc.C2
    assert wps[6][1] == wps[5][1] and wps[9][1] == wps[8][1]                  # ring 2 not pushed in steps 6 and 9
    assert len({w1 - w2 for w1, w2 in wps}) == mc.NSTEP                       # the rings never move in step
    for ring in (1, 2):
        x = mc.RETRY_MS * 1e-3 * mc.RINGS[ring]["f_sf"]
        assert x != round(x), (ring, x)                                       # no whole number in double ...
        assert mc.retry_samples(ring) == mc.RETRY_MS * int(mc.RINGS[ring]["f_sf"]) // 1000   # ... truncated to the exact one
    assert mc.retry_samples(1) != mc.retry_samples(2)
    for spec in mc.MIX:
        assert mc.due_steps(spec, mc.MIX_ACQUIRED_AT[spec[0]]) == mc.MIX_DUE[spec[0]], spec[0]
    by = {s[0]: s for s in mc.MIX}
    assert mc.first_try(by["l1_intg3"]) == 4 * mc.N1 < wps[0][0] < mc.first_try(by["l1_present"]) == 11 * mc.N1
    # were ring 2's retry counted with ring 1's rate, or its channels judged against ring 1, the steps would differ
    wrong = wps[3][1] + mc.retry_samples(1)
    assert [k for k, w in enumerate(wps) if w[1] >= wrong][0] == 7 != mc.MIX_DUE["r2_l1_absent"][1]
    assert wps[1][0] >= mc.first_try(by["r2_l1_present"]) > wps[1][1]
    # ring 2's channels are not due (steps 4..7) while ring 1's already retry (steps 4 and 7)
    assert all(k not in mc.MIX_DUE["r2_l1_absent"] for k in (4, 7))
    # a late satellite's second window is all signal, its first one all noise
    for name, ring in (("l1_late", 1), ("r2_g1_late", 2)):
        f_sf, t_on = mc.RINGS[ring]["f_sf"], by[name][7]
        k1, k2 = mc.MIX_DUE[name]
        assert wps[k1][ring - 1] < t_on * f_sf < wps[k2][ring - 1] - mc.first_try(by[name])


def _search(orc, spec, sig, wp, mk):
    o = mk(orc, spec)
    return ac.oracle_acq(orc, o, sig, sig.shape[0], wp)


def test_mix_scenario_is_decided_by_the_oracle(gc, orc, synth):
    """Every search of the schedule on the oracle, window by window: the outcome claimed, and no decision closer than
    MARGIN to a tie or the threshold.  No search is left out."""
    sig = {r: mc.mix_signal(gc, synth, r) for r in (1, 2)}
    wps = mc.mix_wrpos()
    assert sig[1].shape[0] == wps[-1][0] and sig[2].shape[0] == wps[-1][1]
    jobs, tags = [], []
    for spec in mc.MIX:
        for a, k in enumerate(mc.MIX_DUE[spec[0]]):
            wp = wps[k][spec[3] - 1]
            jobs.append(lambda spec=spec, wp=wp: _search(orc, spec, sig[spec[3]], wp, mc.mix_oracle_channel))
            tags.append((spec, a + 1, k))
    assert len(jobs) == sum(len(v) for v in mc.MIX_DUE.values()) == 15
    for (spec, attempt, k), w in zip(tags, ac.run_oracles(jobs, workers=16)):
        name, acquired_at = spec[0], mc.MIX_ACQUIRED_AT[spec[0]]
        print(name, "attempt", attempt, "step", k, "flagacq", w["flagacq"], "iters", w["iters"], "peakr %.4f" % w["peakr"])
        ac.check_margins(w, (name, attempt))
        assert w["flagacq"] == (1 if attempt == acquired_at else 0), (name, attempt, w["peakr"])
        if w["flagacq"]:
            want = spec[2] * 0.5625e6 * (spec[1] == mc.CTYPE_G1) + mc.RINGS[spec[3]]["f_if"] + spec[5]
            assert abs(w["acqfreq"] - want) <= spec[4][1], (name, w["acqfreq"], want)
        else:
            assert w["iters"] == spec[4][2] and w["peakr"] <= gc.ACQTH, (name, attempt)


def test_hand_scenario_is_decided_by_the_oracle(gc, orc, synth):
    """The hand-over scenario: the listed channels with a satellite are acquired, the two without are not, all with
    the margin; and from the hand-over state the oracle's SBAS channel finds its symbol edge after period 2000 and
    closes its loops at the 2-period interval (flagloopfilter 2) within the periods the device test runs."""
    sig = {r: mc.hand_signal(gc, synth, r) for r in (1, 2)}
    jobs = [lambda s=mc.HAND[i]: _search(orc, s, sig[s[3]], mc.HAND_WRPOS, mc.hand_oracle_channel) for i in mc.HAND_LISTED]
    res = dict(zip(mc.HAND_LISTED, ac.run_oracles(jobs, workers=16)))
    for i, w in res.items():
        print(mc.HAND[i][0], "flagacq", w["flagacq"], "iters", w["iters"], "peakr %.4f" % w["peakr"])
        ac.check_margins(w, mc.HAND[i][0])
        assert w["flagacq"] == (1 if i in mc.HAND_ACQUIRED else 0), mc.HAND[i][0]
    assert abs(res[6]["acqfreq"] - (mc.RTL_OFFSET + 640.0)) <= 200.0 and mc.RTL_OFFSET > 47e3
    o = mc.hand_oracle_channel(orc, mc.HAND[1])
    assert (o.loopms, o.rate, o.ne, o.nl, o.corrn) == (2, 2, 3, 4, 6)
    o.acq.acqfreq = o.carrfreq = res[1]["acqfreq"]
    o.codefreq = o.crate
    ring = orc.make_ring(sig[1], sig[1].shape[0], sig[1].shape[0])
    b = C.c_uint64(res[1]["buffloc"])
    flags = []
    for _ in range(sum(mc.HAND_RUNS)):
        assert orc.lib().orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(b)) == 1
        flags.append(o.flagloopfilter)
    first2 = flags.index(2)
    assert o.flagsync == 1 and 2000 < first2 < 2060, first2
    assert flags[first2:first2 + 6:2] == [2, 2, 2] and flags[first2 + 1:first2 + 6:2] == [0, 0, 0]
    assert abs(o.carrfreq - (4.092e6 - 830.0)) < 30.0, o.carrfreq


def test_synth_t_off_leaves_existing_inputs_byte_identical(gc, synth):
    """make_if without t_off draws as before (the digests of tests/test_rx_host.py); with t_off the satellite is
    unchanged before it and absent from it on, and the other satellites and the noise are untouched."""
    prns = list(range(1, 33))
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in prns}
    s = synth.default_sats(prns, seed=20240601)
    d = synth.make_if(codes, 20 * 16368, f_sf=16.368e6, f_if=0.0, dtype=2, sats=s, seed=20240601)
    assert hashlib.sha256(d.tobytes()).hexdigest() == "16bcfa8e65346eba2f49fcbde5834aa33f51b1a10104d791f53c9968169a133e"
    d1 = synth.make_if(codes, 3 * 16368, f_sf=16.368e6, f_if=4.092e6, dtype=1, sats=s, seed=5, chunk=20000)
    assert hashlib.sha256(d1.tobytes()).hexdigest() == "0609e345687ebf6a8c4b3d66452cdcbe53737a5ae5ccf97a19bef31988acc043"
    n, f_sf = 2 * 16368, 16.368e6
    sat = dict(prn=7, doppler=1000.0, codephase=10.0, cn0=80.0, phase=0.3)
    other = dict(prn=8, doppler=-500.0, codephase=99.0, cn0=45.0, phase=0.1)
    full = synth.make_if(codes, n, f_sf=f_sf, sats=[sat, other], seed=3).astype(np.int32)
    none = synth.make_if(codes, n, f_sf=f_sf, sats=[other], seed=3).astype(np.int32)
    gone = synth.make_if(codes, n, f_sf=f_sf, sats=[dict(sat, t_off=1e-3), other], seed=3).astype(np.int32)
    k = int(np.ceil(1e-3 * f_sf))
    assert np.array_equal(gone[:k], full[:k]) and np.array_equal(gone[k:], none[k:])
    assert not np.array_equal(full[k:], none[k:])
    both = synth.make_if(codes, n, f_sf=f_sf, sats=[dict(sat, t_on=0.5e-3, t_off=1e-3), other], seed=3).astype(np.int32)
    j = int(np.ceil(0.5e-3 * f_sf))
    assert np.array_equal(both[:j], none[:j]) and np.array_equal(both[j:k], full[j:k]) and np.array_equal(both[k:], none[k:])
