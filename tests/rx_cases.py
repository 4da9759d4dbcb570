"""The cold-start scenario of the receiver schedule tests (tests/test_rx_host.py shows on the oracle alone that it is a
real test, tests/test_gpu_rx.py runs it on the device): six GPS L1 C/A channels on 3.5 s of int8 IQ samples at
16.368 Msps -- three satellites present from the start, two never, one switched on after 1 s -- pushed in chunks of
0.25 s with one scheduling step after each chunk, searches retried 1.5 s of samples after a failure."""
import ctypes as C

import numpy as np

F_SF = 16.368e6
NSAMP = 16368
PRNS = [5, 9, 12, 17, 25, 30]               # channel order
PRESENT = {5: (1517.0, 311.3), 12: (-3222.0, 12.8), 25: (4630.0, 870.1)}      # prn: (Doppler Hz, code phase chips)
ABSENT = [9, 17]
LATE, LATE_DOPPLER, LATE_CODEPHASE, LATE_T_ON = 30, -120.0, 555.5, 1.0
CN0 = 47.0
SEED = 311
DURATION = 3.5
CHUNK = int(0.25 * F_SF)                     # samples per push: 250 code periods
NCHUNK = int(DURATION / 0.25)
RETRY_MS = 1500
MAX_PERIODS = 300                            # per step: a chunk's 250 periods and the 11 a new channel starts behind
INTG = 10
FIRST_TRY = (INTG + 1) * NSAMP               # ref src/sdracq.c:24-26
RETRY_SAMPLES = int(RETRY_MS * 1e-3 * F_SF)


def sats():
    rng = np.random.default_rng(SEED)
    out = [dict(prn=p, doppler=d, codephase=c, cn0=CN0, phase=0.4 * i, bits=rng.choice([-1.0, 1.0], size=64))
           for i, (p, (d, c)) in enumerate(PRESENT.items())]
    out.append(dict(prn=LATE, doppler=LATE_DOPPLER, codephase=LATE_CODEPHASE, cn0=CN0, phase=1.1,
                    bits=rng.choice([-1.0, 1.0], size=64), t_on=LATE_T_ON))
    return out


def signal(gc, synth):
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in PRNS}
    return synth.make_if(codes, NCHUNK * CHUNK, f_sf=F_SF, f_if=0.0, dtype=2, sats=sats(), seed=SEED)


def step_wrpos():
    """Write position at each scheduling step."""
    return [CHUNK * (k + 1) for k in range(NCHUNK)]


def due_steps(acquired_at_attempt):
    """Steps (indices into step_wrpos()) at which a channel's search is due when it is acquired at its
    acquired_at_attempt-th search (None: never): the schedule gnsscorr_rx_step must follow."""
    out, next_try = [], FIRST_TRY
    for k, wp in enumerate(step_wrpos()):
        if wp >= next_try:
            out.append(k)
            if acquired_at_attempt is not None and len(out) == acquired_at_attempt:
                break
            next_try = wp + RETRY_SAMPLES
    return out


def oracle_search(orc, o, ring, wrpos):
    """sdracquisition() of the oracle's channel o on the window that ends at wrpos: (returned buffloc, iterations)."""
    ring.wrpos = wrpos
    if not o.xcode:
        o._xc = orc.codespectrum(o)
        o.xcode = o._xc.ctypes.data
    power = np.zeros(o.nfreq * o.nsamp)
    iters = C.c_int()
    buffloc = orc.lib().orc_sdracquisition(C.byref(o), C.byref(ring), power.ctypes.data, C.byref(iters))
    return int(buffloc), iters.value
