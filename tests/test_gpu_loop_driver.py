"""The closed loop's host driver (gnsscorr_loop.hip, below the kernels): what it keeps per channel set (GcLoop).

Two properties no other test pins down: the per-channel write positions are a buffer of their own, whatever the parity
of the channel count, and a channel set configured on a used engine computes in the closed loop what a fresh engine
computes: no buffer, step geometry or tap layout of the earlier set is left behind.  (The earlier set's sizing hints are
reset too, but they only choose kcap, which by design cannot change a result, so no output shows them.)"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_loop import _check_against_oracle, _signal

pytestmark = pytest.mark.gpu
NSAMP = 16368


@pytest.mark.parametrize("nch", [1, 3])
def test_closed_loop_odd_channel_counts(gc, orc, synth, engine, nch):
    """1 and 3 channels (L1CA, int8 IQ, zero IF, 5 taps, filter update every period) on 12 code periods of signal: two
    runs of 4 and 5 periods against the oracle, at test_gpu_loop.py's bar."""
    prns = [5, 12, 25][:nch]
    dop = [1517.0, -3222.0, 4630.0][:nch]
    cph = [311.3, 12.8, 870.1][:nch]
    sig = _signal(gc, synth, prns, dop, cph, 12)
    nsamples = sig.shape[0]
    engine.ring_create(1, 2, nsamples)
    engine.ring_push_raw(1, sig, nsamples)
    chans = [gc.Channel(p, dtype=2, f_if=0.0) for p in prns]
    engine.set_channels(chans)
    ring = orc.make_ring(sig, nsamples, nsamples)
    ochs, bufflocs, states, loops = [], [], [], []
    for i, c in enumerate(chans):
        acqfreq = 200.0 * round(dop[i] / 200.0)
        o = orc.make_chan(c.prn, dtype=2, f_if=0.0)
        o.acq.acqfreq = acqfreq
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = acqfreq, c.crate, 0.0, 0.0
        o.flagsync, o.synci, o.cnt = 0, (3 + 5 * i) % 20, 2001 + 7 * i
        b = int(round((1023 - cph[i]) * 16)) % NSAMP
        ochs.append(o)
        bufflocs.append(C.c_uint64(b))
        states.append(dict(carrfreq=acqfreq, codefreq=c.crate, remcode=0.0, remcarr=0.0, buffloc=b))
        loops.append(engine.loop_state(i, acqfreq, flagsync=0, synci=o.synci, cnt=o.cnt))
    engine.trk_set_state(states)
    engine.loop_set(loops)
    _check_against_oracle(orc, engine, ochs, ring, bufflocs, 4, 5)
    _check_against_oracle(orc, engine, ochs, ring, bufflocs, 5, 5, done=4)
    assert engine.trk_loop_lapped() == 0


def _states(chans, seed):
    rng = np.random.default_rng(seed)
    return [dict(carrfreq=float(rng.uniform(-4000, 4000)), codefreq=c.crate + float(rng.uniform(-2, 2)),
                 remcode=float(rng.uniform(0.01, 0.99)), remcarr=float(rng.uniform(0, 6.2)), buffloc=100 + 900 * i)
            for i, c in enumerate(chans)]


def test_closed_loop_after_reconfiguration_equals_fresh_engine(gc):
    """An engine that ran 2 synchronised channels at loopms 10, then is given 5 channels of a 7-tap layout, computes in
    the closed loop to the bit what a fresh engine with those 5 channels computes."""
    rng = np.random.default_rng(14)
    n = NSAMP * 16
    data = rng.integers(-60, 61, size=(n, 2), dtype=np.int8)
    small = [gc.Channel(p, dtype=2, f_if=0.0) for p in (3, 4)]
    big = [gc.Channel(p, dtype=2, f_if=0.0, corrn=3, corrd=3, corrp=3) for p in (2, 7, 11, 17, 23)]
    live, fresh = gc.Engine(0), gc.Engine(0)
    try:
        for e in (live, fresh):
            e.ring_create(1, 2, n)
            e.ring_push_raw(1, data, n)
        live.set_channels(small)
        live.trk_set_state(_states(small, 23))
        live.loop_set([live.loop_state(i, 500.0, flagsync=1, loop=10) for i in range(len(small))])
        live.trk_run_loop(6)
        live.trk_fetch_log()
        states = _states(big, 21)
        for e in (live, fresh):
            e.set_channels(big)
            e.trk_set_state(states)
            e.loop_set([e.loop_state(i, 200.0 * round(s["carrfreq"] / 200.0), flagsync=0, synci=(7 * i) % 20, cnt=2001)
                        for i, s in enumerate(states)])
        for nrun in (9, 3):
            out = []
            for e in (live, fresh):
                e.trk_run_loop(nrun)
                II, QQ, ns = e.trk_fetch()
                log, ndone = e.trk_fetch_log()
                out.append((II, QQ, ns, log, ndone, e.trk_get_state(), [bytes(l) for l in e.loop_get()], e.trk_loop_lapped()))
            a, b = out
            assert np.all(a[4] == nrun), a[4]
            for k in range(5):
                assert np.array_equal(a[k], b[k]), (nrun, k)
            for f in a[3].dtype.names:
                assert np.array_equal(a[3][f], b[3][f]), (nrun, f)
            assert a[5] == b[5] and a[6] == b[6] and a[7] == b[7], nrun
    finally:
        live.close()
        fresh.close()
