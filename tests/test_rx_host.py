"""Receiver schedule (gnsscorr_rx_*, gnsscorr_acq_run_subset, gnsscorr_loop_start_from_acq), the part that needs no
GPU: the ABI, the synthetic generator's switch-on time, and -- on the CPU oracle alone -- that the cold-start scenario
of tests/test_gpu_rx.py is a real test: a device run that acquired nothing, or everything, could not agree with it."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import rx_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gnsscorr_acq_run_subset", "gnsscorr_loop_start_from_acq", "gnsscorr_rx_start", "gnsscorr_rx_set",
               "gnsscorr_rx_step", "gnsscorr_rx_status"]


def test_rx_symbols_exported_and_declared(gc):
    L = gc.lib()
    hdr = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    for name in NEW_SYMBOLS:
        getattr(L, name)
        assert name in gc.EXPORTS_GNSSCORR and (name + "(") in hdr.replace(" (", "("), name
    assert (gc.CH_IDLE, gc.CH_SEARCH, gc.CH_TRACK) == (0, 1, 2)
    for name, val in (("GNSSCORR_CH_IDLE", 0), ("GNSSCORR_CH_SEARCH", 1), ("GNSSCORR_CH_TRACK", 2)):
        assert any(l.split()[:3] == ["#define", name, str(val)] for l in hdr.splitlines()), name


def test_rxstat_layout(gc, tmp_path):
    """sizeof/offsetof of gnsscorr_rxstat_t compiled from include/gnsscorr.h against the ctypes mirror."""
    fields = ["state", "attempts", "next_try", "acq_wrpos", "acq", "cnt"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gnsscorr.h"\nint main(){printf("%zu", sizeof(gnsscorr_rxstat_t));\n' +
                   "".join('printf(" %%zu", offsetof(gnsscorr_rxstat_t, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals[0] == C.sizeof(gc.RxStat) == 80
    assert vals[1:] == [getattr(gc.RxStat, f).offset for f in fields] == [0, 4, 8, 16, 24, 72]


def test_rx_calls_fail_loudly_without_a_context_state(gc):
    """No schedule without a context: every entry point reports an error instead of crashing."""
    L = gc.lib()
    st = (gc.RxStat * 1)()
    one = (C.c_int * 1)(0)
    assert L.gnsscorr_rx_start(None, 0) == -1
    assert L.gnsscorr_rx_set(None, 0, gc.CH_IDLE) == -3 and L.gnsscorr_rx_step(None, 1) == -3
    assert L.gnsscorr_rx_status(None, st) == -3
    assert L.gnsscorr_acq_run_subset(None, 0, one, 1) == -1 and L.gnsscorr_loop_start_from_acq(None) == -3


def test_synth_t_on_leaves_existing_inputs_byte_identical(gc, synth):
    """make_if without t_on: the same random draws in the same order as before the parameter existed (the digests were
    taken from the generator as it was); with t_on the satellite is absent before it and unchanged after it, and the
    other satellites and the noise are untouched."""
    prns = list(range(1, 33))
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in prns}
    s = synth.default_sats(prns, seed=20240601)
    d = synth.make_if(codes, 20 * 16368, f_sf=16.368e6, f_if=0.0, dtype=2, sats=s, seed=20240601)
    assert hashlib.sha256(d.tobytes()).hexdigest() == "16bcfa8e65346eba2f49fcbde5834aa33f51b1a10104d791f53c9968169a133e"
    d1 = synth.make_if(codes, 3 * 16368, f_sf=16.368e6, f_if=4.092e6, dtype=1, sats=s, seed=5, chunk=20000)
    assert hashlib.sha256(d1.tobytes()).hexdigest() == "0609e345687ebf6a8c4b3d66452cdcbe53737a5ae5ccf97a19bef31988acc043"
    # t_on: one strong satellite on 2 ms, switched on after 1 ms
    n, f_sf = 2 * 16368, 16.368e6
    sat = dict(prn=7, doppler=1000.0, codephase=10.0, cn0=80.0, phase=0.3)
    other = dict(prn=8, doppler=-500.0, codephase=99.0, cn0=45.0, phase=0.1)
    full = synth.make_if(codes, n, f_sf=f_sf, sats=[sat, other], seed=3).astype(np.int32)
    none = synth.make_if(codes, n, f_sf=f_sf, sats=[other], seed=3).astype(np.int32)
    late = synth.make_if(codes, n, f_sf=f_sf, sats=[dict(sat, t_on=1e-3), other], seed=3).astype(np.int32)
    k = int(np.ceil(1e-3 * f_sf))
    assert np.array_equal(late[:k], none[:k]) and np.array_equal(late[k:], full[k:])
    assert not np.array_equal(full[:k], none[:k])


def test_cold_start_scenario_is_decided_by_the_oracle(gc, orc, synth):
    """orc_sdracquisition at the scheduled write positions: every present PRN is acquired at its first due search,
    every absent PRN fails every search (peak ratio <= ACQTH = 3.0), the late PRN fails its first and is acquired at
    its second.  Conditions on the input (seed, C/N0, switch-on time), not tolerances."""
    sig = rc.signal(gc, synth)
    n = sig.shape[0]
    assert n == rc.NCHUNK * rc.CHUNK and rc.NCHUNK == 14
    wps = rc.step_wrpos()
    ring = orc.make_ring(sig, n, n)
    # the schedule itself: first due after the first chunk, retries 1.5 s of samples later
    assert rc.due_steps(None) == [0, 6, 12] and rc.due_steps(1) == [0] and rc.due_steps(2) == [0, 6]
    assert wps[0] >= rc.FIRST_TRY and wps[6] == wps[0] + rc.RETRY_SAMPLES
    assert wps[0] < rc.LATE_T_ON * rc.F_SF < wps[6] - rc.FIRST_TRY          # the late PRN's second window is all signal
    for p in rc.PRNS:
        o = orc.make_chan(p, dtype=2, f_if=0.0)
        assert o.intg == rc.INTG and o.nsamp == rc.NSAMP
        if p in rc.PRESENT:
            buffloc, iters = rc.oracle_search(orc, o, ring, wps[0])
            assert o.flagacq == 1 and o.acq.peakr > gc.ACQTH, (p, o.acq.peakr)
            assert abs(o.acq.acqfreq - rc.PRESENT[p][0]) <= 200.0, (p, o.acq.acqfreq)
            assert wps[0] - rc.FIRST_TRY <= buffloc < wps[0] - rc.FIRST_TRY + rc.NSAMP
        elif p in rc.ABSENT:
            for k in rc.due_steps(None):
                _, iters = rc.oracle_search(orc, o, ring, wps[k])
                assert o.flagacq == 0 and iters == rc.INTG and o.acq.peakr <= gc.ACQTH, (p, k, o.acq.peakr)
        else:
            assert p == rc.LATE
            _, iters = rc.oracle_search(orc, o, ring, wps[0])
            assert o.flagacq == 0 and iters == rc.INTG and o.acq.peakr <= gc.ACQTH, (p, o.acq.peakr)
            rc.oracle_search(orc, o, ring, wps[6])
            assert o.flagacq == 1 and o.acq.peakr > gc.ACQTH, (p, o.acq.peakr)
            assert abs(o.acq.acqfreq - rc.LATE_DOPPLER) <= 200.0
