"""Stream positions past 2^31 and 2^32 on every device path that takes one, against the oracle (parity tests
proper, -m gpu).  At 16.368 Msps sample 2^32 arrives after 4.4 minutes of running: every receiver gets there.

Set-up without pushing 4 G samples: a recording D of R = ringlen samples is pushed, then ring_commit(K*R) advances
the write position to (K+1)*R.  Sample p then holds D[p % R] on the device and in the oracle's
make_ring(D, R, (K+1)*R).  R divides neither 2^31 nor 2^32, so a position truncated to 32 bits (or 31) would land on
another ring slot and read other samples."""
import ctypes as C

import numpy as np
import pytest

import acq_cases as ac
import spec_restate as sr
from conftest import rel_err
from test_gpu_acq_edges import _check as _acq_check, _pair
from test_gpu_loop import _check_against_oracle
from test_gpu_tracking import _oracle_run

pytestmark = pytest.mark.gpu

NS = 16368


def high_layout(T, R0, g, lo, hi):
    """(R, K): R >= R0 a multiple of g that divides neither 2^31 nor 2^32, and K such that the write position
    (K+1)*R lies in [T + lo, T + hi]."""
    R = R0 + (-R0) % g
    while True:
        k1 = -(-(T + lo) // R)
        if k1 * R <= T + hi and (1 << 31) % R and (1 << 32) % R:
            return R, k1 - 1
        R += g


def high_ring(engine, ftype, dtype, D, R, K):
    engine.ring_create(ftype, dtype, R)
    engine.ring_push_raw(ftype, D, R)
    engine.ring_commit(ftype, K * R)
    wp = (K + 1) * R
    assert engine.ring_wrpos(ftype) == wp
    return wp


def _noise(rng, n, dtype):
    return rng.integers(-60, 61, size=(n, 2) if dtype == 2 else (n,), dtype=np.int8)


@pytest.mark.parametrize("T,dtype,f_if", [(1 << 31, 2, 0.0), (1 << 32, 2, 0.0), (1 << 32, 1, 4.092e6)],
                         ids=["2^31_iq", "2^32_iq", "2^32_real"])
def test_batched_tracking_across_high_positions(gc, orc, engine, T, dtype, f_if):
    """trk_run, two consecutive batches of 3 periods (the second planned ahead while the first is correlated), four
    channels that cross position T in different periods of either batch: sums, samples and final state bit for bit."""
    R, K = high_layout(T, 12 * NS, 16 // dtype, 4 * NS, 5 * NS)
    rng = np.random.default_rng(T % 1000 + dtype)
    D = _noise(rng, R, dtype)
    wp = high_ring(engine, 1, dtype, D, R, K)
    prns = [1, 7, 13, 32]
    chans = [gc.Channel(p, dtype=dtype, f_if=f_if, corrn=2, corrd=3, corrp=3) for p in prns]
    engine.set_channels(chans)
    states = [dict(carrfreq=f_if + float(rng.uniform(-5000, 5000)), codefreq=c.crate + float(rng.uniform(-3, 3)),
                   remcode=float(rng.uniform(0, 1)), remcarr=float(rng.uniform(0, 6.2)), buffloc=T - 3 * NS - 6000 + 5000 * i)
              for i, c in enumerate(chans)]
    assert min(s["buffloc"] for s in states) >= wp - R
    engine.trk_set_state(states)
    ochs = [orc.make_chan(p, dtype=dtype, f_if=f_if, corrn=2, corrd=3, corrp=3) for p in prns]
    oII, oQQ, ons, ofin = _oracle_run(orc, ochs, states, D, R, wp, 6)
    ends = np.array([s["buffloc"] for s in states])[:, None] + np.cumsum(ons, axis=1)
    assert np.any(ends[:, 2] <= T) and np.any((ends[:, 1] <= T) & (ends[:, 2] > T)) and np.all(ends[:, 5] > T)
    for b in range(2):
        engine.trk_run(3)
        II, QQ, ns = engine.trk_fetch()
        sl = slice(3 * b, 3 * b + 3)
        assert np.array_equal(ns, ons[:, sl]), b
        assert np.array_equal(II, oII[:, sl]) and np.array_equal(QQ, oQQ[:, sl]), b
    for a, o in zip(engine.trk_get_state(), ofin):
        assert a["remcode"] == o["remcode"] and a["remcarr"] == o["remcarr"] and a["buffloc"] == o["buffloc"]


@pytest.mark.parametrize("T", [1 << 31, 1 << 32], ids=["2^31", "2^32"])
def test_closed_loop_across_high_positions_and_counter(gc, orc, engine, T):
    """trk_run_loop over 17 + 13 periods whose sample positions cross T; four L1 C/A channels after bit sync start at
    period counter cnt = 2^32 - 7 + i (2^32 is no multiple of rate 20: the bit phase of nav_biti's 64-bit branch
    differs from a truncated counter's), the others before sync and after sync at small counters."""
    R, K = high_layout(T, 36 * NS, 8, 20 * NS, 22 * NS)
    rng = np.random.default_rng(T % 977)
    D = _noise(rng, R, 2)
    wp = high_ring(engine, 1, 2, D, R, K)
    ring = orc.make_ring(D, R, wp)
    prns = [3, 8, 12, 19, 21, 27, 30, 32]
    chans = [gc.Channel(p, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3) for p in prns]
    engine.set_channels(chans)
    big = (1 << 32) - 7
    nav = [(1, (3 + 5 * i) % 20, big + i) for i in range(4)] + [(0, 0, 2001), (0, 0, big), (1, 9, 2100), (1, 17, 2345)]
    states, ochs, bufflocs, loops = [], [], [], []
    for i, c in enumerate(chans):
        st = dict(carrfreq=float(rng.uniform(-5000, 5000)), codefreq=c.crate + float(rng.uniform(-3, 3)),
                  remcode=float(rng.uniform(0, 1)), remcarr=float(rng.uniform(0, 6.2)), buffloc=T - 12 * NS + 1000 * i)
        acqfreq = 200.0 * round(st["carrfreq"] / 200.0)
        o = orc.make_chan(c.prn, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3)
        o.acq.acqfreq = acqfreq
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
        o.flagsync, o.synci, o.cnt = nav[i]
        states.append(st)
        ochs.append(o)
        bufflocs.append(C.c_uint64(st["buffloc"]))
        loops.append(engine.loop_state(i, acqfreq, flagsync=nav[i][0], synci=nav[i][1], cnt=nav[i][2]))
    assert min(s["buffloc"] for s in states) >= wp - R
    engine.trk_set_state(states)
    engine.loop_set(loops)
    _check_against_oracle(orc, engine, ochs, ring, bufflocs, 17, 5, tol=1e-12)
    _check_against_oracle(orc, engine, ochs, ring, bufflocs, 13, 5, done=17, tol=1e-12)
    assert all(b.value > T for b in bufflocs) and all(b.value < wp - NS for b in bufflocs)
    fin = engine.trk_get_state()
    lst = engine.loop_get()
    for i, o in enumerate(ochs):
        assert fin[i]["buffloc"] == bufflocs[i].value and fin[i]["remcode"] == o.remcode and fin[i]["remcarr"] == o.remcarr
        for f in ("cnt", "navcnt", "flagsync", "synci", "biti", "swloop", "bit", "swsync", "swreset"):
            assert getattr(lst[i], f) == getattr(o, f), (i, f)
    assert all(lst[i].cnt == big + i + 30 for i in range(4)) and lst[5].cnt == big + 30


def test_acquisition_and_handover_past_2_32(gc, orc, synth, engine):
    """acq_run(wrpos) with wrpos past 2^32 and its search windows across it (a strong, a weak and an absent channel,
    16.368 Msps IQ): flagacq, iters, buffloc, code phase and Doppler bin as the oracle's.  Then trk_start_from_acq
    hands the acquired channels to the loop at their sample index, and 6 periods across 2^32 match the oracle."""
    shape = "16M_iq"
    f_sf, f_if, dtype = ac.C_SHAPES[shape]
    W, n = ac.case_c_span(gc, synth, shape, 41)
    intg = ac.C_GRID[2]
    span = (intg + 1) * n
    T = 1 << 32
    R, K = high_layout(T, 12 * n, 8, 7 * n, 8 * n)
    D = np.concatenate([ac.noise(R - span, dtype, 42), W])
    wp = high_ring(engine, 1, dtype, D, R, K)
    b0 = wp - span
    assert b0 + 2 * n < T < b0 + 5 * n                      # the search windows cross 2^32
    pairs = [_pair(gc, orc, p, dtype, f_sf, f_if, ac.C_GRID) for p in (ac.C_STRONG, ac.C_WEAK, ac.C_ABSENT)]
    chans, ochs = [c for c, _ in pairs], [o for _, o in pairs]
    engine.set_channels(chans)
    keep = [dict(carrfreq=300.0 * i, codefreq=c.crate, remcode=0.5, remcarr=1.0, buffloc=b0 + 4321 * (i + 1))
            for i, c in enumerate(chans)]
    engine.trk_set_state(keep)
    res, wants = _acq_check(engine, orc, chans, ochs, [(D, R, wp)] * 3, wp, power=(0,), where="2^32")
    assert wants[0]["flagacq"] and wants[1]["flagacq"] and not wants[2]["flagacq"]
    assert all(r["buffloc"] >= T - 4 * n for r in res)
    engine.trk_start_from_acq()
    st = engine.trk_get_state()
    tch, bufflocs = [], []
    ring = orc.make_ring(D, R, wp)
    loops = []
    for i, (c, r, s) in enumerate(zip(chans, res, st)):
        want = (dict(carrfreq=r["acqfreq"], codefreq=c.crate, remcode=0.0, remcarr=0.0, buffloc=r["buffloc"])
                if r["flagacq"] else keep[i])
        assert s == want, (i, s, want)
        o = orc.make_chan(c.prn, dtype=dtype, f_sf=f_sf, f_if=f_if)
        o.acq.acqfreq = want["carrfreq"]
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = want["carrfreq"], want["codefreq"], want["remcode"], want["remcarr"]
        o.flagsync, o.synci, o.cnt = 0, 0, 0
        tch.append(o)
        bufflocs.append(C.c_uint64(want["buffloc"]))
        loops.append(engine.loop_state(i, want["carrfreq"]))
    engine.loop_set(loops)
    _check_against_oracle(orc, engine, tch, ring, bufflocs, 6, 5)
    assert all(b.value > T for b in bufflocs) and all(res[i]["buffloc"] < T for i in range(2))


@pytest.mark.parametrize("dtype", [1, 2])
def test_ring_read_and_spectrum_past_2_32(gc, engine, dtype):
    """ring_read and the IF monitor at snapshots past 2^32, one across it, the oldest held and the newest: the samples
    are D's, and histogram and spectrum equal the restatement over them (tolerances of tests/test_gpu_spec.py)."""
    T, N, nfft = 1 << 32, 2 * NS, 16384
    R, K = high_layout(T, 6 * NS, 16 // dtype, 3 * NS, 4 * NS)
    rng = np.random.default_rng(9 + dtype)
    D = _noise(rng, R, dtype)
    wp = high_ring(engine, 1, dtype, D, R, K)
    locs = np.array([T - 1000, wp - R, wp - N, T + 17], np.uint64)
    offs = rng.integers(0, N - nfft // 2 + 1, size=(len(locs), 10)).astype(np.int32)
    freq, pspec, s, hist = engine.spectrum(1, locs, N, NS * 1e3, nfft=nfft, nloop=10, offsets=offs)
    for k, loc in enumerate(locs):
        want = D[(int(loc) + np.arange(N)) % R]
        assert np.array_equal(engine.ring_read(1, int(loc), N, dtype), want), k
        freq_r, pspec_r, s_r = sr.spectrumanalyzer(want, dtype, NS * 1e3, nfft, list(offs[k]))
        yI, yQ = sr.calchistgram(want, dtype, N)
        assert np.array_equal(freq, freq_r)
        assert rel_err(s[k], s_r) < 1e-5, k
        lin = s_r[:nfft] if dtype == 1 else s_r[(np.arange(2 * nfft) + nfft) % (2 * nfft)]
        big = lin >= 1e-4 * lin.max()
        assert np.abs(pspec[k] - pspec_r)[big].max() < 1e-3, k
        assert np.array_equal(hist[k], np.stack([yI, yQ])), k
