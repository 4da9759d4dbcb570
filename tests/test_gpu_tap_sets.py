"""Every correlator tap bucket against the CPU oracle (parity tests proper, -m gpu).

The tracking correlator is compiled once per tap bucket, NTAP = 3, 5, 7, 13, 21 and 33 (launch_corr_taps,
gnsscorr_trk.hip); each instantiation serves the tap counts (lo, NTAP] and masks the accumulator slots it does not
use.  These tests run the lowest and the highest member of every bucket, outermost taps up to the 64 samples
set_channels accepts, every correlator form at 33 taps, full-scale samples at the longest period, the closed loop at
3, 7, 9, 13, 21 and 33 taps (every bucket; 5 taps is what the rest of the suite runs it at) and the reference-named
correlator() with 16 tap pairs.

Bar: bit-exact sums, samples per period, remainders and filter-update flags (tests/test_gpu_tracking.py,
tests/test_gpu_loop.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_loop import _random_states_case
from test_gpu_tracking import _oracle_run, _setup

pytestmark = pytest.mark.gpu

F_SF = 16.368e6
HERE = os.path.dirname(os.path.abspath(__file__))

# (corrn, corrd, corrp): 7, 9, 11, 15, 21, 23 and 33 taps -- the lowest and highest member of every bucket the suite
# did not run yet; outermost taps at 9 .. 64 samples, early/late pairs inner and outermost, one corrp that is no
# multiple of corrd (ne = nl = 0)
TAP_SETS = [(3, 3, 9), (4, 1, 1), (5, 5, 10), (7, 9, 63), (10, 6, 30), (11, 5, 7), (16, 4, 64)]


@pytest.mark.parametrize("dtype,f_if", [(2, 0.0), (1, 4.092e6)])
@pytest.mark.parametrize("taps", TAP_SETS, ids=lambda t: f"{1 + 2 * t[0]}taps")
def test_trk_tap_bucket_matches_oracle(gc, orc, engine, taps, dtype, f_if):
    """Batched trk_run, two consecutive batches of 3 periods (the state chains on the device), 4 channels from
    _setup's mix of start states: sums, samples per period, remainders and the batch sums bit for bit."""
    corrn, corrd, corrp = taps
    nsamples = 16 * 8192
    data, chans, states, ochs = _setup(gc, orc, engine, dtype, f_if, corrn, corrd, corrp, prns=[1, 7, 13, 32],
                                       nsamples=nsamples, seed=500 + corrn, buffloc0=70)
    assert chans[0].ntap == 1 + 2 * corrn and chans[0].corrp[-1] == corrn * corrd
    oII, oQQ, ons, ofin = _oracle_run(orc, ochs, states, data, nsamples, nsamples, 6)
    for b in range(2):
        engine.trk_run(3)
        II, QQ, ns = engine.trk_fetch()
        sl = slice(3 * b, 3 * b + 3)
        assert np.array_equal(ns, ons[:, sl]), b
        assert np.array_equal(II, oII[:, sl]) and np.array_equal(QQ, oQQ[:, sl]), b
        sI, sQ = engine.trk_fetch_sums()
        assert np.array_equal(sI, II.sum(axis=1)) and np.array_equal(sQ, QQ.sum(axis=1)), b
    for a, o in zip(engine.trk_get_state(), ofin):
        assert a["remcode"] == o["remcode"] and a["remcarr"] == o["remcarr"] and a["buffloc"] == o["buffloc"]


def test_tap_span_limits_are_refused_before_anything_runs(gc, orc, engine):
    """An outermost tap at 65 samples and 17 tap pairs are refused by set_channels with GNSSCORR_EINVAL; the
    channels set before stay in force and track as before, bit for bit."""
    nsamples = 16 * 8192
    data, chans, states, ochs = _setup(gc, orc, engine, 2, 0.0, 16, 4, 8, prns=[3, 21], nsamples=nsamples, seed=65,
                                       buffloc0=200)
    L = gc.lib()
    for corrn, corrd, what in ((13, 5, "outermost tap at 65"), (17, 1, "corrn 17")):
        bad = [gc.Channel(p, dtype=2, f_if=0.0, corrn=corrn, corrd=corrd, corrp=corrd) for p in (3, 21)]
        arr = (gc.ChanDesc * 2)(*[c.desc() for c in bad])
        assert L.gnsscorr_set_channels(engine.h, 2, arr) == -1                 # GNSSCORR_EINVAL
        assert what in L.gnsscorr_last_error().decode()
        with pytest.raises(gc.GnsscorrError, match=what):
            engine.set_channels(bad)
    assert engine.channels == chans
    engine.trk_set_state(states)
    engine.trk_run(4)
    II, QQ, ns = engine.trk_fetch()
    oII, oQQ, ons, ofin = _oracle_run(orc, ochs, states, data, nsamples, nsamples, 4)
    assert np.array_equal(ns, ons) and np.array_equal(II, oII) and np.array_equal(QQ, oQQ)
    for a, o in zip(engine.trk_get_state(), ofin):
        assert a["remcode"] == o["remcode"] and a["remcarr"] == o["remcarr"] and a["buffloc"] == o["buffloc"]


# one run of 33 taps with the outermost at 64 samples per dtype, in this process or in a child with another form
FORMS_CASES = [(2, 0.0, 1), (1, 4.092e6, 2)]       # (dtype, f_if, ftype)


def _forms_run(gc, orc, engine, nsamples=16 * 8192, nepoch=5):
    """-> {dtype: (II, QQ, ns, states, data)} for the 33-tap / 64-sample set on both rings."""
    out = {}
    for dtype, f_if, ftype in FORMS_CASES:
        rng = np.random.default_rng(64 + dtype)
        data = rng.integers(-128, 128, size=(nsamples, 2) if dtype == 2 else (nsamples,), dtype=np.int8)
        engine.ring_create(ftype, dtype, nsamples)
        engine.ring_push_raw(ftype, data, nsamples)
        chans = [gc.Channel(p, dtype=dtype, ftype=ftype, f_if=f_if, corrn=16, corrd=4, corrp=12) for p in (2, 9, 17, 30)]
        engine.set_channels(chans)
        states = [dict(carrfreq=f_if + float(rng.uniform(-6000, 6000)), codefreq=c.crate + float(rng.uniform(-4, 4)),
                       remcode=[0.0, 1.0 - 2.0 ** -30, 0.5, float(rng.uniform(0, 1))][i], remcarr=float(rng.uniform(0, 6)),
                       buffloc=64 + 977 * i) for i, c in enumerate(chans)]
        states[0].update(carrfreq=f_if + 2200.0, codefreq=chans[0].crate, remcarr=0.0)
        engine.trk_set_state(states)
        engine.trk_run(nepoch)
        II, QQ, ns = engine.trk_fetch()
        out[dtype] = (II, QQ, ns, states, data)
    return out


def test_all_correlator_forms_agree_at_33_taps(gc, orc, engine, tmp_path):
    """The prefix form (default), the replica form (GNSSCORR_TRK_ALGO=replica), the prefix form without its edge table
    (GNSSCORR_TRK_NOEDGETAB=1) and with one sample per lane and iteration (GNSSCORR_TRK_NIT=1), at 33 taps with the
    outermost at 64 samples, int8 IQ and real samples: all equal to each other and to the oracle, bit for bit.  The
    switches are read once per process, so every other form runs in a child process."""
    nepoch = 5
    base = _forms_run(gc, orc, engine, nepoch=nepoch)
    for dtype, f_if, ftype in FORMS_CASES:
        II, QQ, ns, states, data = base[dtype]
        ochs = [orc.make_chan(p, dtype=dtype, f_if=f_if, corrn=16, corrd=4, corrp=12) for p in (2, 9, 17, 30)]
        oII, oQQ, ons, _ = _oracle_run(orc, ochs, states, data, data.shape[0], data.shape[0], nepoch)
        assert np.array_equal(ns, ons) and np.array_equal(II, oII) and np.array_equal(QQ, oQQ), dtype
    script = tmp_path / "forms.py"
    script.write_text(f"""
import json, sys
sys.path.insert(0, {repr(os.path.dirname(HERE))})
sys.path.insert(0, {repr(HERE)})
import gnsscorr_loader
from test_gpu_tap_sets import _forms_run
gc = gnsscorr_loader.load()
eng = gc.Engine(0)
out = _forms_run(gc, None, eng)
eng.close()
print(json.dumps({{str(k): dict(II=v[0].tolist(), QQ=v[1].tolist(), ns=v[2].tolist()) for k, v in out.items()}}))
""")
    for env_add in (dict(GNSSCORR_TRK_ALGO="replica"), dict(GNSSCORR_TRK_NOEDGETAB="1"), dict(GNSSCORR_TRK_NIT="1")):
        env = dict(os.environ, **env_add)
        out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (env_add, out.stderr[-2000:])
        r = json.loads(out.stdout.strip().splitlines()[-1])
        for dtype in base:
            II, QQ, ns = base[dtype][:3]
            got = r[str(dtype)]
            assert np.array_equal(np.array(got["ns"]), ns), (env_add, dtype)
            assert np.array_equal(np.array(got["II"]), II) and np.array_equal(np.array(got["QQ"]), QQ), (env_add, dtype)


@pytest.mark.parametrize("dtype", [2, 1])
def test_full_scale_samples_33_taps_26msps(gc, orc, engine, dtype):
    """Every sample of the ring an int8 extreme (-128 / -127 / +127), 33 taps, 26 Msps (26000 samples per period, the
    longest the engine runs end to end).  The in-phase rail is channel 0's own code at nominal rate, tracked on a
    carrier of 0 Hz: its prompt sum before the carrier table's 1/32 scale, about 26000 * 128 * 32 = 1.06e8 per period,
    is as large as a period can give, and guards the 32-bit partial and reduction sums of the correlator
    (gnsscorr_ps.h, trk_finish)."""
    f_sf, nper = 26e6, 26000
    nsamples = nper * 8
    rng = np.random.default_rng(127 + dtype)
    code, crate = gc.gencode(1, gc.CTYPE_L1CA)
    k = np.arange(nsamples)
    chip = np.floor(k * (crate / f_sf)).astype(np.int64) % 1023
    rail = np.where(code[chip] > 0, np.int8(-128), np.int8(127))
    rail[rng.random(nsamples) < 0.01] = -127
    if dtype == 2:
        data = np.stack([rail, rng.choice(np.array([-128, -127, 127], np.int8), size=nsamples)], axis=1)
    else:
        data = rail
    engine.ring_create(1, dtype, nsamples)
    engine.ring_push_raw(1, data, nsamples)
    prns = [1, 8, 19, 27]
    chans = [gc.Channel(p, dtype=dtype, f_sf=f_sf, f_if=0.0, corrn=16, corrd=4, corrp=4) for p in prns]
    assert chans[0].nsamp == nper
    engine.set_channels(chans)
    states = [dict(carrfreq=0.0, codefreq=crate, remcode=0.0, remcarr=0.0, buffloc=0)]
    states += [dict(carrfreq=float(rng.uniform(-3000, 3000)), codefreq=c.crate + float(rng.uniform(-2, 2)),
                    remcode=float(rng.uniform(0, 1)), remcarr=float(rng.uniform(0, 6)), buffloc=100 + 3000 * i)
               for i, c in enumerate(chans[1:])]
    engine.trk_set_state(states)
    ochs = [orc.make_chan(p, dtype=dtype, f_sf=f_sf, f_if=0.0, corrn=16, corrd=4, corrp=4) for p in prns]
    oII, oQQ, ons, ofin = _oracle_run(orc, ochs, states, data, nsamples, nsamples, 6)
    # (the reference hands trk.QQ to the correlator as its in-phase output, ref src/sdrtrk.c:42, and scales the sums by
    # 1/32; the integer sums behind channel 0's prompt come to more than 0.95 * 26000 * 128 * 32)
    assert np.abs(oQQ[0, :, 0]).min() > 0.95 * nper * 128
    for b in range(2):
        engine.trk_run(3)
        II, QQ, ns = engine.trk_fetch()
        sl = slice(3 * b, 3 * b + 3)
        assert np.array_equal(ns, ons[:, sl]), b
        assert np.array_equal(II, oII[:, sl]) and np.array_equal(QQ, oQQ[:, sl]), b
    for a, o in zip(engine.trk_get_state(), ofin):
        assert a["remcode"] == o["remcode"] and a["remcarr"] == o["remcarr"] and a["buffloc"] == o["buffloc"]


@pytest.mark.parametrize("taps,flagsync", [
    ((4, 2, 4), 0),             # 9 taps, early/late the inner pair, filter update every period ...
    ((4, 2, 4), 1),             # ... and every 10 periods after nav bit synchronisation
    ((16, 1, 2), 0),            # 33 taps one sample apart, early/late the second pair
    ((16, 1, 2), 1),
    ((4, 2, 3), 1),             # corrp no multiple of corrd: the reference leaves ne = nl = 0 (ref src/sdrinit.c:446-455)
])
def test_closed_loop_9_and_33_taps(gc, orc, engine, taps, flagsync):
    """Closed loop (trk_run_loop) from random start states, teacher-forced as in tests/test_gpu_loop.py: 8 channels x
    100 periods in two runs, int8 IQ at 16.368 Msps, outermost taps at 8 and 16 samples.  (The closed loop at wider
    spans, up to the 64 samples set_channels accepts, on every front end: tests/test_gpu_tap_spans.py.)"""
    corrn, corrd, corrp = taps
    if corrp % corrd:
        c = gc.Channel(1, corrn=corrn, corrd=corrd, corrp=corrp)
        assert c.ne == c.nl == 0 and orc.make_chan(1, corrn=corrn, corrd=corrd, corrp=corrp).ne == 0
    _random_states_case(gc, orc, engine, 900 + 10 * corrn + corrp + flagsync, 2, 0.0, F_SF, taps, flagsync, nper=100,
                        nch=8, chunks=(61, 39))


@pytest.mark.parametrize("taps,flagsync", [
    ((1, 3, 3), 0),             # 3 taps: the bucket of 3
    ((3, 2, 2), 1),             # 7 taps: the bucket of 7
    ((6, 3, 3), 0),             # 13 taps: the bucket of 13
    ((10, 2, 2), 1),            # 21 taps: the bucket of 21
], ids=lambda p: f"{1 + 2 * p[0]}taps" if isinstance(p, tuple) else f"sync{p}")
def test_closed_loop_remaining_tap_buckets(gc, orc, engine, taps, flagsync):
    """The closed loop's correlator instances come off the same tap-bucket ladder as the batch's (trk_with_tap_bucket,
    gnsscorr_ps.h); the cases above and the rest of the suite run it at 5, 9 and 33 taps.  Here 3, 7, 13 and 21 taps,
    the top of the other four buckets: 2 channels x 40 periods in two runs, int8 IQ at 16.368 Msps, before and after
    nav bit synchronisation in turn, bit for bit as above."""
    corrn, corrd, corrp = taps
    _random_states_case(gc, orc, engine, 900 + 10 * corrn + corrp + flagsync, 2, 0.0, F_SF, taps, flagsync, nper=40,
                        nch=2, chunks=(23, 17))


@pytest.mark.parametrize("dtype,freq", [(2, -3456.5), (1, 4.092e6 + 1500.25)])
def test_correlator_symbol_16_tap_pairs_64_samples(gc, orc, dtype, freq):
    """correlator() (ref src/sdrcmn.c:687-722) with 16 tap pairs, the outermost at 64 samples."""
    L = gc.lib()
    rng = np.random.default_rng(16 + dtype)
    n = 16370
    data = rng.integers(-128, 128, size=n * dtype, dtype=np.int8)
    code, crate = gc.gencode(11, gc.CTYPE_L1CA)
    code16 = code.astype(np.int16)
    s = np.arange(4, 65, 4, dtype=np.int32)
    assert len(s) == 16 and s[-1] == 64
    for coff, cr in ((0.0, crate), (511.75, crate + 2.5), (1022.999999, crate - 1.0)):
        II, QQ = np.zeros(33), np.zeros(33)
        remc, remp = C.c_double(), C.c_double()
        L.correlator(data.ctypes.data, dtype, 1 / F_SF, n, freq, 0.3, cr, coff, s.ctypes.data, 16,
                     II.ctypes.data, QQ.ctypes.data, C.byref(remc), C.byref(remp), code16.ctypes.data, 1023)
        oII, oQQ, orc_c, orc_p = orc.correlator(data, dtype, 1 / F_SF, n, freq, 0.3, cr, coff, s, code16)
        assert np.array_equal(II, oII) and np.array_equal(QQ, oQQ), coff
        assert remc.value == orc_c and remp.value == orc_p, coff
