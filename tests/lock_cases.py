"""The loss-of-lock scenario of the lock monitor's tests (tests/test_lock_host.py shows on the oracle alone what it
decides, tests/test_gpu_rx_lock.py runs it on the device): four GPS L1 C/A channels on 8 s of int8 IQ samples at
4.092 Msps, pushed in chunks of 0.25 s with one scheduling step after each chunk.  PRN 5 is always on, PRN 12 is
switched off from 3 s to 5 s, PRN 30 is switched off after 1 s, PRN 9 is absent."""
import ctypes as C

import numpy as np

import lock_restate as lr
import rx_cases as rc

F_SF = 4.092e6
NSAMP = 4092
PRNS = [5, 12, 30, 9]                        # channel order
CN0 = 47.0
SEED = 311
DURATION = 8.0
CHUNK = int(0.25 * F_SF)                     # samples per push: 250 code periods
NCHUNK = int(DURATION / 0.25)
RETRY_MS = 1500
MAX_PERIODS = 300
INTG = 10
FIRST_TRY = (INTG + 1) * NSAMP
RETRY_SAMPLES = int(RETRY_MS * 1e-3 * F_SF)
RATE = 20
CTYPE_L1CA, CTYPE_SBAS = 1, 27
T_OFF_12, T_ON_12, T_OFF_30 = 3.0, 5.0, 1.0
TAPS = dict(corrn=2, corrd=3, corrp=3)       # the receiver's default taps
PRM = dict(sync_periods=2600, kbits=10, nbad=2, mu_min=5.0)
PRM_PRN5 = dict(PRM, sync_periods=6000)      # checksync()'s vote-histogram branch (prn <= 5) synchronises later


def prm_of(prn):
    return PRM_PRN5 if prn == 5 else PRM


def sats():
    rng = np.random.default_rng(SEED)
    bits = [rng.choice([-1.0, 1.0], size=64) for _ in range(3)]
    s12 = dict(prn=12, doppler=-3222.0, codephase=12.8, cn0=CN0, phase=0.4, bits=bits[1])
    return [dict(prn=5, doppler=1517.0, codephase=311.3, cn0=CN0, phase=0.0, bits=bits[0]),
            dict(s12, t_off=T_OFF_12), dict(s12, t_on=T_ON_12),
            dict(prn=30, doppler=-120.0, codephase=555.5, cn0=CN0, phase=1.1, bits=bits[2], t_off=T_OFF_30)]


def signal(gc, synth):
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in PRNS}
    return synth.make_if(codes, NCHUNK * CHUNK, f_sf=F_SF, f_if=0.0, dtype=2, sats=sats(), seed=SEED)


def channels(gc, prns=PRNS):
    return [gc.Channel(p, dtype=2, f_sf=F_SF, f_if=0.0, **TAPS) for p in prns]


def step_wrpos():
    return [CHUNK * (k + 1) for k in range(NCHUNK)]


def schedule_step(ch, wp, lost_word, search):
    """The schedule rule of one channel for one step (gnsscorr_rx_step's parts 0 to 2).  ch: dict(state, next_try,
    attempts, losses), updated; lost_word: the monitor's verdict of the previous step; search(wp) -> acquired, called
    when the channel's search is due.  States: 1 SEARCH, 2 TRACK."""
    if lost_word and ch["state"] == 2:
        ch["state"], ch["next_try"] = 1, wp
        ch["losses"] += 1
    if ch["state"] == 1 and wp >= ch["next_try"] and wp >= FIRST_TRY:
        ch["attempts"] += 1
        if search(wp):
            ch["state"] = 2
        else:
            ch["next_try"] = wp + RETRY_SAMPLES
        return True
    return False


def oracle_schedule(gc, orc, sig, prn, prm, ctype=CTYPE_L1CA, rate=RATE, taps=TAPS, wrpos=None, keep_rows=False):
    """The scenario of one channel on the oracle alone, free-running: orc_sdracquisition whenever the schedule rule makes
    a search due, orc_sdrthread_step for up to MAX_PERIODS periods per step while TRACK, the restated detector over each
    step's periods.  ctype, rate: the channel's code type and the periods of its nav bit (L1 C/A: 20, SBAS: 2); wrpos: the
    write position at each step (default: step_wrpos()).  Returns dict(steps=[per step: state, attempts, losses, searched,
    peakr, flagacq, ndone, cnt, lost_word], events=[(kind, step, cnt, value)], sync=[cnt at which each run synchronised],
    runs=number of hand-overs, lost_t=[stream time in seconds of each losing period], handover=[buffloc of each
    hand-over]); with keep_rows also rows=[per step: dict(run, cnt0, navbit, buffloc)], run counting the hand-overs."""
    L = orc.lib()
    n = sig.shape[0]
    ring = orc.make_ring(sig, n, 0)
    mk = lambda: orc.make_chan(prn, ctype=ctype, dtype=2, f_sf=F_SF, f_if=0.0, **taps)
    box = dict(o=mk(), buffloc=C.c_uint64(0))
    ch = dict(state=1, next_try=FIRST_TRY, attempts=0, losses=0)
    st = lr.zero_state()
    out = dict(steps=[], events=[], sync=[], runs=0, lost_t=[], handover=[], rows=[])
    lost_word = 0

    def search(wp):
        o = box["o"] = mk()                                     # the hand-over leaves a fresh channel (cnt = 0)
        b, _ = rc.oracle_search(orc, o, ring, wp)
        box["buffloc"] = C.c_uint64(b)
        box["peakr"] = o.acq.peakr
        if o.flagacq:
            out["runs"] += 1
            out["sync"].append(None)
            out["handover"].append(b)
        return bool(o.flagacq)

    for k, wp in enumerate(step_wrpos() if wrpos is None else wrpos):
        box["peakr"] = None
        searched = schedule_step(ch, wp, lost_word, search)
        o = box["o"]
        rows = dict(I=[], Q=[], fs=[], nb=[], b=[])
        cnt0 = int(o.cnt)
        if ch["state"] == 2:
            ring.wrpos = wp
            while len(rows["I"]) < MAX_PERIODS:
                rows["b"].append(int(box["buffloc"].value))             # first sample of the period
                if not L.orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(box["buffloc"])):
                    break
                rows["I"].append(o.II[0])
                rows["Q"].append(o.QQ[0])
                rows["fs"].append(o.flagsync)
                rows["nb"].append(o.bit if (o.flagsync and o.swsync) else 0)
                if o.flagsync and out["sync"][-1] is None:
                    out["sync"][-1] = int(o.cnt) - 1
        ev = []
        lr.run(st, prm, rate, rows["I"], rows["Q"], rows["fs"], rows["nb"], len(rows["I"]), cnt0, events=ev)
        lost_word = int(any(e[0] == "lost" for e in ev))
        out["events"] += [(e[0], k, e[1], e[2]) for e in ev]
        out["lost_t"] += [rows["b"][e[1] - cnt0] / F_SF for e in ev if e[0] == "lost"]
        if keep_rows:
            nd = len(rows["I"])
            out["rows"].append(dict(run=out["runs"], cnt0=cnt0, navbit=np.array(rows["nb"], np.int32),
                                    buffloc=np.array(rows["b"][:nd], np.uint64)))
        out["steps"].append(dict(state=ch["state"], attempts=ch["attempts"], losses=ch["losses"], searched=searched,
                                 peakr=box["peakr"], flagacq=int(o.flagacq), ndone=len(rows["I"]), cnt=int(o.cnt),
                                 lost_word=lost_word, next_try=ch["next_try"]))
    return out
