"""The reference's RTL-SDR and GN3S v2 front ends against the CPU oracle (parity tests proper, -m gpu).

frontend/rtlsdr_L1.ini: 2.048 Msps int8 IQ, zero IF, CORRN=4 CORRD=1 CORRP=1 (9 taps one sample apart): the
shortest period (nsamp = 2048, nsampchip = 2) and a chip step of 1023/2048, just below the 0.5 binade edge.
frontend/gn3sv2_L1.ini: 8.1838 Msps int8 IQ, IF 38.4 kHz, CORRN=6 CORRD=2 CORRP=2 (13 taps): a period of 8183.8
samples (nsamp = 8183, odd; nsampchip = 7, which sets checkacquisition()'s exclusion window) and a chip step just
above the 0.125 binade edge.

Bars as in tests/test_gpu_acq.py (decisions identical, power / peak ratio / C/N0 to 1e-4), tests/test_gpu_tracking.py
and tests/test_gpu_loop.py (sums, samples, remainders and filter-update flags bit for bit; filter outputs
teacher-forced)."""
import ctypes as C

import numpy as np
import pytest

from acq_cases import _cn0_restated
from conftest import rel_err
from test_gpu_loop import _check_against_oracle
from test_gpu_tracking import _oracle_run

pytestmark = pytest.mark.gpu

# the shipped front-end files' values (loop bandwidths [before, after] nav bit synchronisation)
FRONTENDS = {
    "rtlsdr": dict(f_sf=2.048e6, f_if=0.0, taps=(4, 1, 1), nsamp=2048, nsampchip=2, edge=0.5,
                   dllb=(5.0, 2.0), pllb=(30.0, 20.0), fllb=(200.0, 50.0)),
    "gn3sv2": dict(f_sf=8.1838e6, f_if=38.4e3, taps=(6, 2, 2), nsamp=8183, nsampchip=7, edge=0.125,
                   dllb=(5.0, 1.0), pllb=(30.0, 10.0), fllb=(200.0, 50.0)),
}
FE_IDS = list(FRONTENDS)


def _chans(gc, orc, fe, prns, **kw):
    corrn, corrd, corrp = fe["taps"]
    chans = [gc.Channel(p, dtype=2, f_sf=fe["f_sf"], f_if=fe["f_if"], corrn=corrn, corrd=corrd, corrp=corrp, **kw)
             for p in prns]
    ochs = [orc.make_chan(p, dtype=2, f_sf=fe["f_sf"], f_if=fe["f_if"], corrn=corrn, corrd=corrd, corrp=corrp,
                          dllb=fe["dllb"], pllb=fe["pllb"], fllb=fe["fllb"], **kw) for p in prns]
    assert chans[0].nsamp == ochs[0].nsamp == fe["nsamp"] and chans[0].nsampchip == ochs[0].nsampchip == fe["nsampchip"]
    return chans, ochs


def _loop_state(engine, fe, i, acqfreq, o):
    return engine.loop_state(i, acqfreq, dllb=fe["dllb"], pllb=fe["pllb"], fllb=fe["fllb"], flagsync=o.flagsync,
                             synci=o.synci, cnt=o.cnt)


def _ringlen(n):
    """n samples rounded up to whole 16-byte groups of int8 IQ (gnsscorr_ring_create)"""
    return (n + 7) // 8 * 8


def _signal(gc, synth, fe, sats, nsamples, seed):
    codes = {s["prn"]: gc.gencode(s["prn"], gc.CTYPE_L1CA) for s in sats}
    return synth.make_if(codes, nsamples, f_sf=fe["f_sf"], f_if=fe["f_if"], dtype=2, sats=sats, seed=seed)


def _codefreq_for_step(ti, step):
    """A code frequency f with ti * f == step exactly in fp64 (the chip step of the reference's rescode(), ref
    src/sdrcmn.c:608-621)."""
    f = step / ti
    for _ in range(64):
        p = ti * f
        if p == step:
            return f
        f = np.nextafter(f, np.inf if p < step else -np.inf)
    raise AssertionError(step)


def _acquire(orc, ochs, data, wrpos):
    ring = orc.make_ring(data, data.shape[0], wrpos)
    out = []
    for o in ochs:
        xc = orc.codespectrum(o)
        o.xcode = xc.ctypes.data
        power = np.zeros(o.nfreq * o.nsamp)
        iters = C.c_int()
        buffloc = orc.lib().orc_sdracquisition(C.byref(o), C.byref(ring), power.ctypes.data, C.byref(iters))
        o.xcode = None
        out.append((buffloc, iters.value, power))
    return out


def _check_acq(r, o, buffloc, iters, where):
    assert r["flagacq"] == o.flagacq, (where, r, o.acq.peakr)
    assert r["iters"] == iters and r["buffloc"] == buffloc, where
    assert r["acqcodei"] == o.acq.acqcodei and r["freqi"] == o.acq.freqi and r["acqfreq"] == o.acq.acqfreq, where
    assert abs(r["peakr"] - o.acq.peakr) <= 1e-4 * o.acq.peakr, where
    assert abs(r["cn0"] - o.acq.cn0) <= 1e-4 * abs(o.acq.cn0), where


@pytest.mark.parametrize("name", FE_IDS)
def test_acquisition_matches_oracle(gc, orc, synth, engine, name):
    """Three PRNs (two present, one absent), a write position that is no multiple of the period, the full power array
    of one present channel."""
    fe = FRONTENDS[name]
    nsamp = fe["nsamp"]
    rng = np.random.default_rng(len(name))
    sats = [dict(prn=p, doppler=float(rng.uniform(-4000, 4000)), codephase=float(rng.uniform(0, 1023)), cn0=47.0,
                 phase=float(rng.uniform(0, 6.28)), bits=rng.choice([-1.0, 1.0], size=32)) for p in (4, 23)]
    nsamples = _ringlen(14 * nsamp)
    data = _signal(gc, synth, fe, sats, nsamples, seed=70 + nsamp)
    engine.ring_create(1, 2, nsamples)
    engine.ring_push_raw(1, data, nsamples)
    prns = [4, 15, 23]
    chans, ochs = _chans(gc, orc, fe, prns)
    engine.set_channels(chans)
    wrpos = 12 * nsamp + 1001
    engine.acq_run(wrpos)
    res = engine.acq_fetch()
    for i, (o, (buffloc, iters, power)) in enumerate(zip(ochs, _acquire(orc, ochs, data, wrpos))):
        _check_acq(res[i], o, buffloc, iters, prns[i])
        assert res[i]["flagacq"] == (prns[i] != 15), prns[i]
        # the exclusion window (nsampchip = 2 / 7): device and oracle C/N0 each against the restatement over their own
        # power at the decisive iteration, to 1e-9
        P = engine.acq_power(i)
        assert P.shape == (o.nfreq, nsamp)
        want = _cn0_restated(P, res[i]["acqcodei"], res[i]["freqi"], chans[i].nsampchip, chans[i].ctime)
        assert abs(res[i]["cn0"] - want) <= 1e-9 * abs(want), (prns[i], res[i]["cn0"], want)
        want = _cn0_restated(power.reshape(o.nfreq, nsamp), o.acq.acqcodei, o.acq.freqi, fe["nsampchip"], o.ctime)
        assert abs(o.acq.cn0 - want) <= 1e-9 * abs(want), (prns[i], o.acq.cn0, want)
        if prns[i] == 23:
            s = sats[1]
            assert abs(res[i]["acqfreq"] - fe["f_if"] - s["doppler"]) <= 200.0
            assert rel_err(P.ravel(), power) <= 1e-4


@pytest.mark.parametrize("name", FE_IDS)
def test_batched_tracking_matches_oracle(gc, orc, engine, name):
    """8 channels x two batches of 64 periods on noise: random mid-track states, remcode exactly 0 and within 1e-6 of
    1 chip, and code frequencies whose chip step is the binade edge itself (f_sf/2 at 2.048 Msps, f_sf/8 at 8.1838 Msps)
    and one ulp either side -- legal states, though no DLL would hold them."""
    fe = FRONTENDS[name]
    nsamp, nepoch = fe["nsamp"], 64
    rng = np.random.default_rng(300 + nsamp)
    nsamples = _ringlen(nsamp * (2 * nepoch + 8))
    data = rng.integers(-128, 128, size=(nsamples, 2), dtype=np.int8)
    engine.ring_create(1, 2, nsamples)
    engine.ring_push_raw(1, data, nsamples)
    prns = [2, 6, 11, 17, 20, 24, 29, 31]
    chans, ochs = _chans(gc, orc, fe, prns)
    engine.set_channels(chans)
    ti = chans[0].ti
    edge = _codefreq_for_step(ti, fe["edge"])
    assert edge == fe["f_sf"] * fe["edge"]                  # (f_sf/2 and f_sf/8 are exact)
    below = _codefreq_for_step(ti, np.nextafter(fe["edge"], 0.0))
    above = _codefreq_for_step(ti, np.nextafter(fe["edge"], 1.0))
    states = []
    for i, c in enumerate(chans):
        states.append(dict(carrfreq=fe["f_if"] + float(rng.uniform(-6000, 6000)),
                           codefreq=[edge, below, above][i] if i < 3 else c.crate + float(rng.uniform(-5, 5)),
                           remcode=[0.0, 1.0 - float(rng.uniform(0, 1e-6)), 0.0, float(rng.uniform(0, 1e-6))][i % 4]
                           if i < 6 else float(rng.uniform(0, 1)),
                           remcarr=float(rng.uniform(0, 6.2)) if i % 3 else 0.0, buffloc=int(rng.integers(0, nsamp))))
    states[3].update(carrfreq=fe["f_if"] + 1400.0, codefreq=chans[3].crate, remcode=0.0, remcarr=0.0)  # fresh from acq
    engine.trk_set_state(states)
    oII, oQQ, ons, ofin = _oracle_run(orc, ochs, states, data, nsamples, nsamples, 2 * nepoch)
    for b in range(2):
        engine.trk_run(nepoch)
        II, QQ, ns = engine.trk_fetch()
        sl = slice(b * nepoch, (b + 1) * nepoch)
        assert np.array_equal(ns, ons[:, sl]), b
        assert np.array_equal(II, oII[:, sl]) and np.array_equal(QQ, oQQ[:, sl]), b
    for a, o in zip(engine.trk_get_state(), ofin):
        assert a["remcode"] == o["remcode"] and a["remcarr"] == o["remcarr"] and a["buffloc"] == o["buffloc"]


@pytest.mark.parametrize("name", FE_IDS)
def test_closed_loop_through_bit_sync(gc, orc, synth, engine, name):
    """Three satellites with 50 bps data from the state sdracquisition() leaves (ref src/sdracq.c:51-55), the shipped
    loop bandwidths: filter update every period until checksync() finds the bit edge (from cnt 2000 on, ref
    src/sdrnav.c:30; PRNs above 5 use the sign shift register), then every 10 periods -- 360 periods in three runs,
    teacher-forced as in tests/test_gpu_loop.py."""
    fe = FRONTENDS[name]
    nsamp, nper = fe["nsamp"], 360
    f_sf, f_if = fe["f_sf"], fe["f_if"]
    prns, dop, cph = [9, 17, 26], [1517.0, -3222.0, 2630.0], [311.3, 12.8, 870.1]
    rng = np.random.default_rng(nsamp)
    sats = [dict(prn=p, doppler=d, codephase=c, cn0=50.0, phase=0.3 * i, bits=rng.choice([-1.0, 1.0], size=64))
            for i, (p, d, c) in enumerate(zip(prns, dop, cph))]
    nsamples = _ringlen(nsamp * (nper + 4))
    sig = _signal(gc, synth, fe, sats, nsamples, seed=11 + nsamp)
    engine.ring_create(1, 2, nsamples)
    engine.ring_push_raw(1, sig, nsamples)
    chans, ochs = _chans(gc, orc, fe, prns)
    engine.set_channels(chans)
    ring = orc.make_ring(sig, nsamples, nsamples)
    bufflocs, states, loops = [], [], []
    for i, (c, o) in enumerate(zip(chans, ochs)):
        acqfreq = f_if + 200.0 * round(dop[i] / 200.0)
        o.acq.acqfreq = acqfreq
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = acqfreq, c.crate, 0.0, 0.0
        o.flagsync, o.synci, o.cnt = 0, 0, 1950 + 13 * i
        b = int(round((1023 - cph[i]) * f_sf / c.crate)) % nsamp        # the first sample of a code period
        bufflocs.append(C.c_uint64(b))
        states.append(dict(carrfreq=acqfreq, codefreq=c.crate, remcode=0.0, remcarr=0.0, buffloc=b))
        loops.append(_loop_state(engine, fe, i, acqfreq, o))
    engine.trk_set_state(states)
    engine.loop_set(loops)
    ntap = chans[0].ntap
    done = 0
    for nrun in (1, 150, 209):
        _check_against_oracle(orc, engine, ochs, ring, bufflocs, nrun, ntap, done=done, tol=1e-12)
        done += nrun
    lst = engine.loop_get()
    for i, o in enumerate(ochs):
        assert o.flagsync == 1 and lst[i].flagsync == 1, i            # loop-1 -> bit sync -> loop-10 on every channel
        for f in ("synci", "biti", "navcnt", "swloop", "bit", "cnt"):
            assert getattr(lst[i], f) == getattr(o, f), (i, f)
        assert abs(o.carrfreq - (f_if + dop[i])) < 150.0, (i, o.carrfreq)


def test_rtlsdr_file_replay_end_to_end(gc, orc, synth, engine):
    """RTL-SDR file replay (FEND = FILERTLSDR, PPMERR = 30): unsigned bytes through ring_push_packed, acquisition on the
    grid shifted by foffset = f_cf*30e-6 = 47262.6 Hz (ref src/sdrinit.c:616-617, :632-635), the hand-over on the
    device (trk_start_from_acq) and the closed loop, whose DLL carrier aiding subtracts foffset (ref src/sdrtrk.c:147-148)
    -- against the oracle's expander, sdracquisition() and thread loop."""
    fe = FRONTENDS["rtlsdr"]
    nsamp, nper = fe["nsamp"], 300
    prns, dop, cph = [7, 13, 30], [2130.0, -1460.0, 0.0], [402.6, 977.2, 0.0]       # PRN 30 absent
    chans, ochs = _chans(gc, orc, fe, prns, fend=gc.FEND_FRTLSDR, ppmerr=30)
    foff = 1575.42e6 * 30 * 1e-6
    assert all(c.foffset == o.foffset == foff for c, o in zip(chans, ochs))
    sats = [dict(prn=p, doppler=foff + d, codephase=c, cn0=49.0, phase=0.5 * i, bits=np.ones(8))
            for i, (p, d, c) in enumerate(zip(prns[:2], dop, cph))]
    nsamples = nsamp * (nper + 16)
    sig = _signal(gc, synth, fe, sats, nsamples, seed=2048)
    raw = np.clip(sig.astype(np.int16).reshape(-1) + 128, 0, 255).astype(np.uint8)
    data = np.zeros(2 * nsamples, np.int8)
    orc.lib().orc_rtlsdr_exp(raw.ctypes.data, 2 * nsamples, data.ctypes.data)
    data = data.reshape(nsamples, 2)
    engine.ring_create(1, 2, nsamples)
    engine.ring_push_packed(gc.FMT_RTLSDR, raw, nsamples)
    engine.set_channels(chans)
    wrpos = 11 * nsamp + 517
    engine.acq_run(wrpos)
    res = engine.acq_fetch()
    parked = dict(carrfreq=foff, codefreq=chans[0].crate, remcode=0.5, remcarr=0.0, buffloc=100)
    engine.trk_set_state([dict(parked) for _ in chans])
    engine.trk_start_from_acq()
    got = engine.trk_get_state()
    bufflocs, loops = [], []
    for i, (o, (buffloc, iters, _)) in enumerate(zip(ochs, _acquire(orc, ochs, data, wrpos))):
        _check_acq(res[i], o, buffloc, iters, prns[i])
        assert res[i]["flagacq"] == (prns[i] != 30), prns[i]
        if o.flagacq:
            assert abs(o.acq.acqfreq - foff - dop[i]) <= 200.0, i
            st = dict(carrfreq=o.carrfreq, codefreq=o.codefreq, remcode=0.0, remcarr=0.0, buffloc=buffloc)
        else:
            o.acq.acqfreq = foff
            o.carrfreq, o.codefreq, o.remcode, o.remcarr = parked["carrfreq"], parked["codefreq"], 0.5, 0.0
            st = parked
        assert got[i] == st, (i, got[i], st)
        o.flagsync, o.synci, o.cnt = 0, 0, 0
        bufflocs.append(C.c_uint64(st["buffloc"]))
        loops.append(_loop_state(engine, fe, i, o.acq.acqfreq, o))
    engine.loop_set(loops)
    ring = orc.make_ring(data, nsamples, nsamples)
    _check_against_oracle(orc, engine, ochs, ring, bufflocs, 120, chans[0].ntap, tol=1e-12)
    _check_against_oracle(orc, engine, ochs, ring, bufflocs, 180, chans[0].ntap, done=120, tol=1e-12)
    for i in range(2):
        assert abs(ochs[i].carrfreq - (foff + dop[i])) < 150.0, (i, ochs[i].carrfreq)
