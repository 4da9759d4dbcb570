"""First batches of freshly made engines vs the oracle, and results that must not depend on what device memory held
before (-m gpu, except the last test).

Two ways a fresh engine can go wrong without the parity tests noticing: an owned ring whose zero fill is still
running when the first samples arrive on the ingest stream (a window of the pushed samples comes back as zeros),
and a kernel that reads an element of its scratch that no kernel wrote (whatever the previous owner of the memory
left there).  The first is checked where it is most likely to show -- a 1 GiB ring written at its far end right
after it was made; the second deterministically, with gnsscorr_debug_poison filling every scratch buffer with a
chosen byte before its first use.  Bar: bit-exact, as in test_gpu_tracking.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SF = 16.368e6
NSAMP = 16368


def _oracle_periods(orc, ochs, ring, bufflocs, nepoch, ntap):
    """nepoch further periods of every channel from the oracle's current state (sdrtracking, ref src/sdrtrk.c)."""
    L = orc.lib()
    II = np.zeros((len(ochs), nepoch, ntap))
    QQ = np.zeros_like(II)
    ns = np.zeros((len(ochs), nepoch), np.int32)
    for i, o in enumerate(ochs):
        for e in range(nepoch):
            L.orc_sdrtracking(C.byref(o), C.byref(ring), bufflocs[i])
            assert o.flagtrk == 1
            II[i, e] = np.ctypeslib.as_array(o.II)[:ntap]
            QQ[i, e] = np.ctypeslib.as_array(o.QQ)[:ntap]
            ns[i, e] = o.currnsamp
            bufflocs[i] += o.currnsamp
    return II, QQ, ns


def _oracle_channels(orc, chans, states, dtype, f_if, f_sf, taps):
    ochs = []
    for c, st in zip(chans, states):
        o = orc.make_chan(c.prn, dtype=dtype, f_if=f_if, f_sf=f_sf, corrn=taps[0], corrd=taps[1], corrp=taps[2])
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
        ochs.append(o)
    return ochs


def _sweep_states(rng, chans, f_if, dopp, dcode, nsamp):
    """Starting states as tools/debug/plan_sweep.py chooses them: remcode 0, just above 0, just below 1 chip and
    mid-chip; the extreme carrier and code offsets exactly on two channels; one channel on the acquisition grid."""
    states = []
    for i, c in enumerate(chans):
        edge = i % 5
        remcode = (0.0 if edge == 0 else float(rng.uniform(0.0, 1e-6)) if edge == 1 else
                   float(1.0 - rng.uniform(0.0, 1e-6)) if edge == 2 else float(rng.uniform(0.01, 0.99)))
        states.append(dict(carrfreq=f_if + float(rng.uniform(-dopp, dopp)),
                           codefreq=c.crate + float(rng.uniform(-dcode, dcode)),
                           remcode=remcode, remcarr=float(rng.uniform(0, 6.2831)) if i % 7 else 0.0,
                           buffloc=int(rng.integers(0, nsamp))))
    states[0].update(carrfreq=f_if + dopp, codefreq=chans[0].crate + dcode)
    states[1].update(carrfreq=f_if - dopp, codefreq=chans[1].crate - dcode)
    states[3].update(carrfreq=f_if + 200.0 * round(rng.uniform(-30, 30)), codefreq=chans[3].crate)
    return states


# ---------------------------------------------------------------------------------------------------------------
# a. the ring written just after it was created
# ---------------------------------------------------------------------------------------------------------------
BIG = 1 << 29               # samples: an IQ ring of 1 GiB, whose zero fill takes longest to reach its end


def _warm_ingest(engine):
    # on a fresh context the first push allocates the pinned staging buffers, which would delay its first copy
    # well past the zero fill of a ring made just before
    engine.ring_create(1, 2, 1 << 16)
    engine.ring_push_raw(1, np.ones((1 << 12, 2), np.int8), 1 << 12)


@pytest.mark.gpu
def test_ring_push_right_after_create_lands(gc, engine):
    _warm_ingest(engine)
    n = 1 << 20
    data = np.random.default_rng(31).integers(-128, 128, size=(n, 2), dtype=np.int8)
    engine.ring_create(1, 2, BIG)
    engine.ring_commit(1, BIG - n)           # the last samples of the ring: where the zero fill ends
    engine.ring_push_raw(1, data, n)
    got = engine.ring_read(1, BIG - n, n, 2)
    assert np.array_equal(got, data), int(np.count_nonzero(np.any(got != data, axis=1)))


@pytest.mark.gpu
def test_ring_push_packed_right_after_create_lands(gc, orc, engine):
    _warm_ingest(engine)
    n = 1 << 20
    raw = np.random.default_rng(32).integers(0, 256, size=2 * n, dtype=np.uint8)
    exp = np.zeros(2 * n, np.int8)
    orc.lib().orc_rtlsdr_exp(raw.ctypes.data, 2 * n, exp.ctypes.data)
    engine.ring_create(1, 2, BIG)
    engine.ring_commit(1, BIG - n)
    engine.ring_push_packed(gc.FMT_RTLSDR, raw, n)
    got = engine.ring_read(1, BIG - n, n, 2).reshape(-1)
    assert np.array_equal(got, exp), int(np.count_nonzero(got != exp))


@pytest.mark.gpu
def test_ring_recreated_while_a_push_is_in_flight(gc, engine):
    """A ring made again while 16 MB are still on their way into the old one: the new ring holds the second push
    and zeros after it, nothing of the first."""
    _warm_ingest(engine)
    rng = np.random.default_rng(33)
    n1, n2, ringlen = 1 << 23, 1 << 20, 1 << 23                # 16 MB, 2 MB; IQ ring of 16 MB
    a = rng.integers(1, 128, size=(n1, 2), dtype=np.int8)      # no zero byte: any survivor shows
    b = rng.integers(-128, 128, size=(n2, 2), dtype=np.int8)
    engine.ring_create(1, 2, ringlen)
    engine.ring_push_raw(1, a, n1)
    engine.ring_create(1, 2, ringlen)
    engine.ring_push_raw(1, b, n2)
    assert engine.ring_wrpos(1) == n2
    assert np.array_equal(engine.ring_read(1, 0, n2, 2), b)
    rest = engine.ring_read(1, n2, ringlen - n2, 2)
    assert not rest.any(), int(np.count_nonzero(np.any(rest != 0, axis=1)))


# ---------------------------------------------------------------------------------------------------------------
# b. the whole first batch of a fresh engine at the shape of the sweep's configuration 103
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_first_batches_of_a_fresh_poisoned_engine_32_channels_13_taps(gc, orc):
    """32 channels, IQ at 16.368 Msps, 13 taps, Doppler to +-10 kHz, code to +-12 chips/s, on an engine whose
    scratch starts out as 0xA5 bytes, in the order create -> push -> set_channels -> set_state -> run.  Batch 1
    (500 periods) is planned from the state just set; batch 2 (100) is planned afresh and plans batch 3 ahead,
    from claims discovered ahead: every channel-period of the three against the oracle."""
    taps = (6, 3, 6)
    ntap = 1 + 2 * taps[0]
    batches = (500, 100, 100)
    rng = np.random.default_rng(103)
    nsamples = NSAMP * (sum(batches) + 14)
    data = rng.integers(-60, 61, size=(nsamples, 2), dtype=np.int8)
    data.reshape(-1)[:4] = [-128, 127, -128, 127]
    eng = gc.Engine(0)
    try:
        eng.debug_poison(0xA5)
        eng.ring_create(1, 2, nsamples)
        eng.ring_push_raw(1, data, nsamples)
        chans = [gc.Channel(1 + (p % 32), dtype=2, f_if=0.0, f_sf=F_SF, corrn=taps[0], corrd=taps[1], corrp=taps[2])
                 for p in range(32)]
        eng.set_channels(chans)
        states = _sweep_states(rng, chans, 0.0, 10000.0, 12.0, NSAMP)
        eng.trk_set_state(states)
        ochs = _oracle_channels(orc, chans, states, 2, 0.0, F_SF, taps)
        ring = orc.make_ring(data, nsamples, nsamples)
        bufflocs = [st["buffloc"] for st in states]
        for b, nepoch in enumerate(batches):
            eng.trk_run(nepoch)
            II, QQ, ns = eng.trk_fetch()
            sI, sQ = eng.trk_fetch_sums()
            oII, oQQ, ons = _oracle_periods(orc, ochs, ring, bufflocs, nepoch, ntap)
            bad = np.argwhere(np.any(II != oII, axis=2) | np.any(QQ != oQQ, axis=2) | (ns != ons))
            assert bad.size == 0, (b, len(bad), bad[:8].tolist())
            assert np.array_equal(sI, II.sum(axis=1)) and np.array_equal(sQ, QQ.sum(axis=1)), b
            fin = eng.trk_get_state()
            for i, (f, o) in enumerate(zip(fin, ochs)):
                assert f["remcode"] == o.remcode and f["remcarr"] == o.remcarr and f["buffloc"] == bufflocs[i], (b, i)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------
# c. results do not depend on the earlier contents of device memory
# ---------------------------------------------------------------------------------------------------------------
C_TAPS = (2, 3, 3)
C_NEPOCH = 120
C_F_IF = 4.092e6


def _case_c(gc):
    """16 channels of real samples at 4.092 MHz IF (the other front end of the sweep), 5 taps."""
    rng = np.random.default_rng(2024)
    nsamples = NSAMP * 330                     # also room for the 300-period batches of the engines in between
    data = rng.integers(-60, 61, size=nsamples, dtype=np.int8)
    chans = [gc.Channel(1 + (3 * p) % 32, dtype=1, f_if=C_F_IF, f_sf=F_SF, corrn=C_TAPS[0], corrd=C_TAPS[1],
                        corrp=C_TAPS[2]) for p in range(16)]
    states = _sweep_states(rng, chans, C_F_IF, 10000.0, 12.0, NSAMP)
    return data, chans, states


def _fresh_run(gc, poison):
    """A fresh engine (poison byte, or None: off) through case c's two batches: everything it returns."""
    data, chans, states = _case_c(gc)
    eng = gc.Engine(0)
    try:
        if poison is not None:
            eng.debug_poison(poison)
        eng.ring_create(1, 1, data.shape[0])
        eng.ring_push_raw(1, data, data.shape[0])
        eng.set_channels(chans)
        eng.trk_set_state(states)
        out = []
        for _ in range(2):
            eng.trk_run(C_NEPOCH)
            out += list(eng.trk_fetch()) + list(eng.trk_fetch_sums())
        out.append(np.array([[f["remcode"], f["remcarr"], f["buffloc"]] for f in eng.trk_get_state()]))
    finally:
        eng.close()
    return out


def _other_engine(gc, nch, taps, nepoch, poison):
    """An engine of another size that runs one batch and is closed: it leaves its results in memory the next
    engine's buffers may be carved from."""
    data, chans, states = _case_c(gc)
    eng = gc.Engine(0)
    try:
        if poison is not None:
            eng.debug_poison(poison)
        eng.ring_create(1, 1, data.shape[0])
        eng.ring_push_raw(1, data, data.shape[0])
        chans = [gc.Channel(c.prn, dtype=1, f_if=C_F_IF, f_sf=F_SF, corrn=taps[0], corrd=taps[1], corrp=taps[2])
                 for c in (chans * 2)[:nch]]
        eng.set_channels(chans)
        eng.trk_set_state((states * 2)[:nch])
        eng.trk_run(nepoch)
        eng.trk_fetch()
    finally:
        eng.close()


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y), (what, k)


@pytest.mark.gpu
def test_results_do_not_depend_on_earlier_memory_contents(gc, orc, tmp_path):
    ref = _fresh_run(gc, 0x00)
    # equal to the oracle once
    data, chans, states = _case_c(gc)
    ntap = 1 + 2 * C_TAPS[0]
    ochs = _oracle_channels(orc, chans, states, 1, C_F_IF, F_SF, C_TAPS)
    ring = orc.make_ring(data, data.shape[0], data.shape[0])
    bufflocs = [st["buffloc"] for st in states]
    for b in range(2):
        oII, oQQ, ons = _oracle_periods(orc, ochs, ring, bufflocs, C_NEPOCH, ntap)
        II, QQ, ns, sI, sQ = ref[5 * b:5 * b + 5]
        assert np.array_equal(ns, ons) and np.array_equal(II, oII) and np.array_equal(QQ, oQQ), b
        assert np.array_equal(sI, II.sum(axis=1)) and np.array_equal(sQ, QQ.sum(axis=1)), b
    fin = ref[-1]
    for i, o in enumerate(ochs):
        assert fin[i, 0] == o.remcode and fin[i, 1] == o.remcarr and fin[i, 2] == bufflocs[i], i
    # ... and bit-identical whatever the scratch held
    for poison in (0xFF, 0xA5):
        _assert_same(_fresh_run(gc, poison), ref, poison)
    _other_engine(gc, 32, (6, 3, 6), 300, 0x5A)
    _other_engine(gc, 7, (1, 8, 8), 50, None)
    _other_engine(gc, 24, (2, 3, 3), 200, None)
    _assert_same(_fresh_run(gc, None), ref, "poison off, after other engines")
    # the independent correlator form and the older planner chain, each in a process of its own (the library reads
    # its environment switches once)
    ref_path = tmp_path / "ref.npz"
    np.savez(ref_path, *ref)
    script = tmp_path / "child.py"
    script.write_text(f"""
import sys
import numpy as np
sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]
import gnsscorr_loader
import test_gpu_fresh_state as t
out = t._fresh_run(gnsscorr_loader.load(), 0xA5)
np.savez(sys.argv[1], *out)
""")
    for env_add in (dict(GNSSCORR_TRK_ALGO="replica"), dict(GNSSCORR_TRK_NOSPEC="1")):
        out_path = tmp_path / "child.npz"
        env = dict(os.environ, **env_add)
        r = subprocess.run([sys.executable, str(script), str(out_path)], env=env, capture_output=True, text=True,
                           timeout=180)
        assert r.returncode == 0, (env_add, r.stderr[-2000:])
        z = np.load(out_path)
        _assert_same([z[f"arr_{k}"] for k in range(len(ref))], ref, env_add)


@pytest.mark.gpu
def test_poison_byte_out_of_range_is_refused(gc, engine):
    for bad in (-2, 256):
        with pytest.raises(gc.GnsscorrError):
            engine.debug_poison(bad)
    engine.debug_poison(0x00)
    engine.debug_poison(-1)


# ---------------------------------------------------------------------------------------------------------------
# d. the first closed-loop call and the first acquisition of a poisoned fresh engine
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def poisoned(gc):
    e = gc.Engine(0)
    e.debug_poison(0xA5)
    yield e
    e.close()


@pytest.mark.gpu
def test_closed_loop_on_a_poisoned_fresh_engine(gc, orc, synth, poisoned):
    from test_gpu_loop import _run_case
    _run_case(gc, orc, synth, poisoned, 2, 0.0, 2, 3, 3, nper=220, flagsync=0, chunks=(1, 100, 119))


@pytest.mark.gpu
def test_acquisition_on_a_poisoned_fresh_engine(gc, orc, synth, poisoned):
    from test_gpu_acq import test_acquisition_matches_oracle as acquisition_case
    acquisition_case(gc, orc, synth, poisoned, 2, 0.0)


# ---------------------------------------------------------------------------------------------------------------
# e. no device needed
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0, -1])
def test_debug_poison_null_context(gc, byte):
    assert gc.lib().gnsscorr_debug_poison(None, byte) == -1          # GNSSCORR_EINVAL
