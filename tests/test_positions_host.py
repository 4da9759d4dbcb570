"""Stream positions and period counters past 2^31 and 2^32 in host code (no GPU): the premise of
tests/test_gpu_positions.py, and the observables / frame replays of a closed-loop log at such positions against the
oracle's setobsdata() / frame synchronisation."""
import ctypes as C

import numpy as np
import pytest

from lnav_frames import l1ca_subframe

NS = 16368


@pytest.mark.parametrize("T", [1 << 31, 1 << 32])
@pytest.mark.parametrize("dtype,f_if", [(2, 0.0), (1, 4.092e6)])
def test_oracle_at_p_plus_KR_equals_p(orc, T, dtype, f_if):
    """A ring of R samples whose write position was advanced by K*R (ring_commit) holds D[p % R] at sample p: the
    oracle's thread steps from p + K*R equal those from p, bit for bit (sums, samples, remainders, filters, nav)."""
    R = 12 * NS + 1000
    assert (1 << 31) % R and (1 << 32) % R
    K = T // R - 1                                              # T - K*R in [R, 2R)
    rng = np.random.default_rng(T % 101 + dtype)
    D = rng.integers(-60, 61, size=(R, 2) if dtype == 2 else (R,), dtype=np.int8)
    hi = orc.make_ring(D, R, (K + 3) * R)
    lo = orc.make_ring(D, R, 3 * R)
    L = orc.lib()
    for k in range(3):
        p = T - K * R - 3 * NS + 1111 * k
        oc = []
        for _ in range(2):
            o = orc.make_chan(5 + k, dtype=dtype, f_if=f_if, corrn=2, corrd=3, corrp=3)
            o.acq.acqfreq = o.carrfreq = f_if + 1400.0 - 600.0 * k
            o.codefreq, o.remcode, o.remcarr = o.crate + 0.7, 0.3, 1.1
            o.flagsync, o.synci, o.cnt = k % 2, 4, 2001
            oc.append(o)
        bh, bl = C.c_uint64(p + K * R), C.c_uint64(p)
        assert bh.value < T < bh.value + 5 * NS                  # (the steps cross T)
        for e in range(10):
            assert L.orc_sdrthread_step(C.byref(oc[0]), C.byref(hi), C.byref(bh)) == 1
            assert L.orc_sdrthread_step(C.byref(oc[1]), C.byref(lo), C.byref(bl)) == 1
            a, b = oc
            assert a.currnsamp == b.currnsamp and a.remcode == b.remcode and a.remcarr == b.remcarr, (k, e)
            assert list(a.II)[:5] == list(b.II)[:5] and list(a.QQ)[:5] == list(b.QQ)[:5], (k, e)
            assert a.carrfreq == b.carrfreq and a.codefreq == b.codefreq and a.flagloopfilter == b.flagloopfilter, (k, e)
            assert bh.value - bl.value == K * R


@pytest.mark.parametrize("base", [(1 << 31) - 170, (1 << 32) - 170])
def test_observables_replayed_at_high_positions(gc, orc, base):
    """gnsscorr_obs_replay with sample indices, period counters and the frame's first period counter past 2^31 /
    2^32 (the counter crosses it during the replay) against orc_setobsdata called inside the oracle's thread loop."""
    NP = 420
    rng = np.random.default_rng(base % 1009)
    data = rng.integers(-40, 41, size=((NP + 4) * NS, 2), dtype=np.int8)
    ring = orc.make_ring(data, data.shape[0], 1 << 40)          # (samples are read at buffloc % length)
    o = orc.make_chan(3, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3)
    o.acq.acqfreq = o.carrfreq = 1200.0
    o.codefreq = o.crate
    o.remcode, o.remcarr = 0.25, 1.5
    o.flagacq = 1
    o.flagsync, o.synci, o.cnt, o.prn = 1, 7, base, 3
    st = gc.ObsState()
    st.f_sf, st.f_if, st.foffset, st.ctime, st.loopms = o.f_sf, o.f_if, o.foffset, o.ctime, o.loopms
    st.oldremcode = o.remcode
    st.firstsftow, st.firstsfcnt = 345600.0, base - 1500
    o.firstsftow, o.firstsfcnt = 345600.0, base - 1500
    log = np.zeros(NP, dtype=np.dtype(gc.TrkLog))
    II0 = np.zeros(NP)
    want = []
    buffloc = C.c_uint64((base << 4) + 11)                        # past 2^35: sample index at 16 samples per count
    for p in range(NP):
        n_before = o.obs_n
        b0 = buffloc.value
        assert orc.lib().orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(buffloc)) == 1
        log[p]["carrfreq"], log[p]["codefreq"] = o.carrfreq, o.codefreq
        log[p]["remcode"], log[p]["remcarr"] = o.remcode, o.remcarr
        log[p]["buffloc"], log[p]["currnsamp"], log[p]["flagloopfilter"] = b0, o.currnsamp, o.flagloopfilter
        II0[p] = o.II[0]
        if o.obs_n != n_before:
            want.append((o.obs_tow, o.obs_remcout, o.obs_L, o.obs_D, o.obs_S if o.obs_Isum == 0.0 else None, o.obs_codei,
                         o.obs_cntout))
    assert len(want) >= 40 and want[0][6] < (base + 170) < want[-1][6]
    rows = list(gc.obs_replay(st, log[:200], II0[:200], cnt0=base))
    rows += list(gc.obs_replay(st, log[200:], II0[200:], cnt0=base + 200))
    assert len(rows) == len(want)
    for r, w in zip(rows, want):
        assert (r["tow"], r["remcout"], r["L"], r["D"], int(r["codei"]), int(r["cntout"])) == (w[0], w[1], w[2], w[3], w[5], w[6])
        assert (r["snr"] == 1 and r["S"] == w[4]) if w[4] is not None else r["snr"] == 0


@pytest.mark.parametrize("cnt0", [(1 << 31) - 24000, (1 << 32) - 24000])
def test_frame_replay_at_high_counters(gc, orc, cnt0):
    """gnsscorr_frame_replay on decided bits whose period counters cross 2^31 / 2^32 between the ends of the first and
    the second subframe, and whose sample indices lie past 2^32: preamble, parity, hand-over word and the frame's first
    period / sample as the oracle's orc_navframe_l1ca, bit by bit."""
    rng = np.random.default_rng(cnt0 % 997)
    bits = [int(x) for x in rng.choice([-1, 1], size=777)]
    prev2 = [bits[-2], bits[-1]]
    for k in range(2):
        sf, prev2 = l1ca_subframe(rng, prev2, 45678 + k, 1 + k, 1)
        bits += sf
    bits += [int(x) for x in rng.choice([-1, 1], size=40)]
    nper = 7 + 20 * len(bits)
    log = np.zeros(nper, dtype=np.dtype(gc.TrkLog))
    for i, bv in enumerate(bits):
        log[7 + 20 * i]["navbit"] = bv
        log[7 + 20 * i]["buffloc"] = (1 << 33) + 16368 * (7 + 20 * i)
    of = orc.Frame()
    st = gc.FrameState()
    done = 0
    for chunk in (4000, 9000, nper - 13000):
        gc.frame_replay(st, log[done:done + chunk], cnt0=cnt0 + done)
        for p in range(done, done + chunk):
            orc.lib().orc_navframe_l1ca(C.byref(of), int(log[p]["navbit"]), int(log[p]["buffloc"]), cnt0 + p)
        done += chunk
        assert list(st.fbits) == list(of.fbits)
        for f in ("polarity", "flagsyncf", "flagtow", "flagdec", "sfid", "firstsf", "firstsfcnt", "firstsftow", "tow_gpst"):
            assert getattr(st, f) == getattr(of, f), (done, f)
    first_end = 7 + 20 * (777 + 300 - 1)
    assert st.flagtow == 1 and st.firstsfcnt == cnt0 + first_end and st.firstsf == (1 << 33) + 16368 * first_end
    assert st.flagdec == 1 and st.firstsftow == 45678 * 6.0 and st.tow_gpst == 45679 * 6.0
