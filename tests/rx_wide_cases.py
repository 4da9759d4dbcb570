"""The wide receiver of the schedule-stage tests (tests/test_rx_wide_host.py shows on the CPU oracle alone that the
scenario decides what it claims, tests/test_gpu_rx_wide.py runs it on the device).  Not a conftest.

Eleven channels on two rings, shaped like BASELINE configs[3], with the lock monitor, bit synchronisation by symbol
energy and the correlation monitor on together through gnsscorr_rx_step: the only path that builds its rows view with a
mapped channel list, rate / cnt at the stride of gnsscorr_loop_t, cnt0 = cnt - ndone and the correlator's own sums at
row_stride = ntap (gc_rows_of_run, csrc/gnsscorr_stage.h).  The scenario is there to make that path run with lists
that are long (three workgroups, the last one partial), sparse (list index != channel), ragged (0 rows beside 250)
and different from stage to stage.

  ring 1  int8 IQ, 2.048 Msps, zero IF (the front end of bsync_cases / cfm_cases): five L1 C/A satellites, PRN 9 absent.
  ring 2  int8 IQ, 4.092 Msps, zero IF (the front end of lock_cases / lock_sbas_cases): two L1 C/A satellites, SBAS
          PRN 120 and 133 with the symbols of lock_sbas_cases, PRN 22 absent.

L1 C/A bits are tied to the code (synth.make_if, symbol_periods 20) and alternate, as in cfm_cases.

Step k = 0 .. 11 pushes 0.25 s of ring 1 and, except in the steps R2_SKIP, 0.25 s of ring 2, then one
gnsscorr_rx_step(300).  A ring 2 channel has caught up with its ring behind every step, so in a step of R2_SKIP it
stays in TRACK with 0 rows beside ring 1 channels with 250 rows (three chunks of 64 and one of 58).

Channel order: see CH.  Every four consecutive channels mix the rings; SBAS 120 sits between two L1 C/A channels.

What happens to whom (asserted on the oracle by the host test, frozen in EXPECT_STATES):
  Y = channel 5 (PRN 7)   its signal ends at T_OFF; the lock monitor's windows of 5 bits drop below mu_min and it is
                          lost by reason 2, searched once more in vain and left in SEARCH (RETRY_MS reaches past the end).
  X = channel 7 (PRN 17)  bit synchronisation off at first and sync_periods 500: lost by reason 1 at cnt 499 in step 2,
                          acquired again in step 3 with cnt restarting at 0.  Parked before step 4 while all its stage
                          states are still zero (no flagsync yet), sent to SEARCH before step 6 and acquired a third time.
                          Before step 6 it also gets bit synchronisation and a sync_periods it can meet: with the detector
                          off for X throughout, at most eight channels could ever be in its list, and the third workgroup
                          of rx_bsync (list entries 8 ..) would never launch.  Step 6 skips ring 2: the nine-entry lists
                          of the lock monitor and the detector run there with 0 rows beside 250.
  channel 6 (SBAS 133)    correlation monitor off: a gap in the middle of that stage's channel range.
  the absent PRNs         searched at step 0 and RETRY_MS later, which is a different step on each ring."""
import ctypes as C

import numpy as np

import bsync_cases as bc
import bsync_restate as br
import cfm_restate as cr
import lock_cases as lc
import lock_restate as lr
import lock_sbas_cases as ls
import rx_cases as rc

CH_IDLE, CH_SEARCH, CH_TRACK = 0, 1, 2
CTYPE_L1CA, CTYPE_SBAS = lc.CTYPE_L1CA, lc.CTYPE_SBAS
F_CF, CRATE, CLEN = 1575.42e6, 1.023e6, 1023
RINGS = {1: dict(f_sf=bc.F_SF, nsamp=bc.NSAMP), 2: dict(f_sf=lc.F_SF, nsamp=lc.NSAMP)}
CHUNK = {r: int(0.25 * RINGS[r]["f_sf"]) for r in RINGS}     # samples per push: 250 code periods
NSTEP = 12                                                   # 3 s
R2_SKIP = (4, 6)                # steps without a ring 2 push: 4 is inside the 33-tap run, 6 has all nine channels in TRACK
MAX_PERIODS = 300
RETRY_MS = 1500                 # a failed search waits 6 pushes of its own ring: one retry per absent PRN, none for Y
INTG = 10
TAPS = dict(corrn=2, corrd=1, corrp=1)                       # 5 taps
TAPS33 = dict(corrn=16, corrd=1, corrp=1)                    # 33 taps: row_stride 33, 16 pairs
NSTEP33 = 6                                                  # the 33-tap run: 1.5 s
NBITS = 160
T_OFF = 1.6                     # Y's signal ends inside step 6; two windows of 0.1 s on noise follow: lost in step 7

# (name, ring, ctype, prn, Doppler Hz, code phase chips, C/N0 dB-Hz, carrier phase); Doppler None: absent.  PRNs above 5
# throughout: checksync()'s shift-register branch, which synchronises behind cnt 2000 within the recording (cadence run).
# Dopplers lie off the 200 Hz search grid by various amounts, code phases are those the suite uses elsewhere plus a few.
CH = [
    ("r1_a", 1, CTYPE_L1CA, 12, -1130.0, 311.3, 48.0, 0.4),
    ("r2_sbas120", 2, CTYPE_SBAS, 120, 2210.0, 640.7 + 1023.0, 47.0, 0.7),
    ("r1_b", 1, CTYPE_L1CA, 23, 2105.0, 640.7, 47.0, 1.9),
    ("r2_a", 2, CTYPE_L1CA, 14, 1517.0, 311.3, 47.0, 0.0),
    ("r1_absent", 1, CTYPE_L1CA, 9, None, None, None, None),
    ("r1_off", 1, CTYPE_L1CA, 7, 517.0, 12.8, 50.0, 3.3),
    ("r2_sbas133", 2, CTYPE_SBAS, 133, -1240.0, 311.3, 47.0, 1.1),
    ("r1_nobsync", 1, CTYPE_L1CA, 17, -2660.0, 870.1, 48.0, 2.5),
    ("r2_absent", 2, CTYPE_L1CA, 22, None, None, None, None),
    ("r1_c", 1, CTYPE_L1CA, 26, 3310.0, 100.2, 49.0, 5.1),
    ("r2_b", 2, CTYPE_L1CA, 30, -120.0, 555.5, 48.0, 1.1),
]
NCH = len(CH)
Y, X, CFM_GAP = 5, 7, 6
PRESENT = [i for i, s in enumerate(CH) if s[4] is not None]
ABSENT = [i for i, s in enumerate(CH) if s[4] is None]
RING_OF = [s[1] for s in CH]
RATES = [2 if s[2] == CTYPE_SBAS else 20 for s in CH]
SEED = {1: 1711, 2: 1712}

# ---- the stages --------------------------------------------------------------------------------------------------------
# lock monitor, on for all.  L1 C/A: windows of 5 bits (0.1 s), so that Y is lost within 0.3 s of T_OFF; mu_min as in
# lock_cases.  SBAS: the window and threshold of lock_sbas_cases.  sync_periods 1000: the detector presets every channel
# behind cnt 718 (L1 C/A) or 400 (SBAS).  X starts with 500, which no channel without the detector can meet.
LOCK_L1 = dict(sync_periods=1000, kbits=5, nbad=2, mu_min=5.0)
LOCK_SBAS = dict(sync_periods=1000, kbits=ls.KBITS, nbad=ls.NBAD, mu_min=ls.MU_MIN)
LOCK_X0 = dict(LOCK_L1, sync_periods=500)
# bit synchronisation: the parameters DESIGN.md 3.2g derives for the two rates
BSYNC_L1, BSYNC_SBAS = bc.PRM, bc.SBAS_PRM
# correlation monitor: two gnsscorr_rx_cfm_set calls.  LOOSE (channels 0 .. 5): no window can be bad but by a prompt
# sum that is not positive.  TIGHT (channels 7 .. 10): the reference shape of ring 1 (taps at 1 and 2 samples, a chip is
# 2: early + late = prompt at pair 1).  On ring 2 a chip is 4 samples and pair 1 gives 1.5: every window of channel 10
# is bad by 0.5 against rtol 0.1, the alarm is certain.
CFM_LOOSE = dict(kbits=4, skip_bits=10, nbad=2, npair=2, dtol=1e3, rtol=1e3, dref=(0.0, 0.0), rref=(1.0, 0.0))
CFM_TIGHT = dict(kbits=5, skip_bits=3, nbad=2, npair=1, dtol=0.2, rtol=0.1, dref=(0.0,), rref=(1.0,))
CFM_SETS = [(0, 6, CFM_LOOSE), (7, 4, CFM_TIGHT)]
# the 33-tap run lasts 1.5 s: fewer bits skipped, all 16 pairs tested on the first set; X is parked before it could
# synchronise, so the second set starts behind it
CFM_SETS33 = [(0, 6, dict(CFM_LOOSE, skip_bits=2, npair=16, dref=(0.0,) * 16, rref=(1.0,) + (0.0,) * 15)),
              (8, 3, dict(CFM_TIGHT, skip_bits=2))]
# the cadence run (lock and correlation monitors only): thresholds nothing fails and no time limit
LOCK_NEVER = dict(sync_periods=0, kbits=5, nbad=10 ** 6, mu_min=1.5)
ALL_STAGES = ("lock", "bsync", "cfm")


def initial_prm(stages=ALL_STAGES, cfm_sets=None, lock_of=None):
    """Per stage the parameters of every channel at gnsscorr_rx_start (None: off)."""
    cfm_sets = CFM_SETS if cfm_sets is None else cfm_sets
    p = dict(lock=[None] * NCH, bsync=[None] * NCH, cfm=[None] * NCH)
    for i, s in enumerate(CH):
        sbas = s[2] == CTYPE_SBAS
        if "lock" in stages:
            p["lock"][i] = lock_of(i) if lock_of else (LOCK_X0 if i == X else (LOCK_SBAS if sbas else LOCK_L1))
        if "bsync" in stages and i != X:
            p["bsync"][i] = BSYNC_SBAS if sbas else BSYNC_L1
    if "cfm" in stages:
        for ch0, n, q in cfm_sets:
            for i in range(ch0, ch0 + n):
                p["cfm"][i] = q
    return p


# What the host does between the steps, before the push of step k: ("rx_set", channel, state) or (stage, channel,
# parameters).  A stage's entry is dropped on an engine that runs without that stage.
COMMANDS = {4: [("rx_set", X, CH_IDLE)],
            6: [("rx_set", X, CH_SEARCH), ("bsync", X, BSYNC_L1), ("lock", X, LOCK_L1)]}
PARKED_STEPS = (4, 5)

# The state of every channel behind each step, S(EARCH) / T(RACK) / I(DLE): what the schedule rule gives from the
# oracle's verdicts (tests/test_rx_wide_host.py asserts it) and what the device must show.
EXPECT_STATES = {0: "TTTTTTTTTTTT", 1: "TTTTTTTTTTTT", 2: "TTTTTTTTTTTT", 3: "TTTTTTTTTTTT", 4: "SSSSSSSSSSSS",
                 5: "TTTTTTTTSSSS", 6: "TTTTTTTTTTTT", 7: "TTTTIITTTTTT", 8: "SSSSSSSSSSSS", 9: "TTTTTTTTTTTT",
                 10: "TTTTTTTTTTTT"}
EXPECT_LOSSES = {X: [(2, 1)], Y: [(7, 2)]}       # channel: [(step of the verdict, reason)]


def wrpos(nstep=NSTEP):
    """[(write position of ring 1, of ring 2)] behind the pushes of each step."""
    out, w2 = [], 0
    for k in range(nstep):
        if k not in R2_SKIP:
            w2 += CHUNK[2]
        out.append((CHUNK[1] * (k + 1), w2))
    return out


def first_try(ring):
    return (INTG + 1) * RINGS[ring]["nsamp"]


def retry_samples(ring):
    return int(RETRY_MS * 1e-3 * RINGS[ring]["f_sf"])


def schedule_step(ch, wp, lost_word, search, ring):
    """lock_cases.schedule_step, which knows ring 2's constants, for a channel of either ring: ring 1's first try is
    earlier than ring 2's and both lie before the first push ends, so only the pause of a failed search differs."""
    assert max(first_try(1), first_try(2)) == lc.FIRST_TRY <= min(CHUNK[1], CHUNK[2])
    searched = lc.schedule_step(ch, wp, lost_word, search)
    if searched and ch["state"] == CH_SEARCH:
        ch["next_try"] = wp + retry_samples(ring)
    return searched


def l1_bits():
    return np.where(np.arange(NBITS) % 2 == 0, 1.0, -1.0)


def sats(ring, keep_on=False):
    out = []
    for i, (name, r, ctype, prn, dop, cph, cn0, ph) in enumerate(CH):
        if r != ring or dop is None:
            continue
        d = dict(prn=name, doppler=dop, codephase=cph, cn0=cn0, phase=ph)
        if ctype == CTYPE_SBAS:
            d.update(bits=ls.symbols().astype(np.float64), symbol_periods=2)
        else:
            d.update(bits=l1_bits(), symbol_periods=20)
        if i == Y and not keep_on:
            d["t_off"] = T_OFF
        out.append(d)
    return out


_SIGNALS = {}


def signal(gc, synth, ring, keep_on=False):
    """The recording of one ring, generated once per process: 3 s of ring 1; 2.75 s of ring 2, of which the scenario
    pushes 2.5 s and the cadence run all.  keep_on: Y's signal does not end (ring 1 only differs)."""
    key = (ring, bool(keep_on) and ring == 1)
    if key not in _SIGNALS:
        codes = {s[0]: gc.gencode(s[3], s[2]) for s in CH if s[1] == ring and s[4] is not None}
        n = NSTEP * CHUNK[1] if ring == 1 else (NSTEP - 1) * CHUNK[2]
        _SIGNALS[key] = synth.make_if(codes, n, f_sf=RINGS[ring]["f_sf"], f_if=0.0, dtype=2, sats=sats(ring, key[1]),
                                      seed=SEED[ring])
    return _SIGNALS[key]


def channels(gc, taps=TAPS):
    return [gc.Channel(s[3], ctype=s[2], dtype=2, ftype=s[1], f_sf=RINGS[s[1]]["f_sf"], f_if=0.0, **taps) for s in CH]


def code_period(i, buffloc):
    """The code period of the absolute code phase that starts at the hand-over sample `buffloc` of channel i."""
    _, ring, _, _, dop, cph, _, _ = CH[i]
    x = (cph + CRATE * (1.0 + dop / F_CF) * buffloc / RINGS[ring]["f_sf"]) / CLEN
    assert abs(x - round(x)) < 0.02, (i, x)      # the hand-over is on a code epoch to a few hundredths of a period
    return int(round(x))


def true_synci(i, buffloc):
    return br.layout_synci(code_period(i, buffloc), 0, RATES[i])


def lists(states, prm):
    """Per stage the channel list of a step's launch: the TRACK channels that have the stage on, ascending (GcStage::fill)."""
    return {s: [i for i in range(NCH) if prm[s][i] is not None and states[i] == CH_TRACK] for s in ALL_STAGES}


def groups(lst):
    return [lst[a:a + 4] for a in range(0, len(lst), 4)]


def ragged(lst, ndone):
    """A workgroup of the list that holds a channel with 0 rows beside one with 250."""
    return any(any(ndone[i] == 0 for i in g) and any(ndone[i] == 250 for i in g) for g in groups(lst))


def apply_commands(prm, k, stages, commands=None):
    """The commands before step k on the parameter table `prm` (updated); returns them as (kind, channel, value) with
    the entries of stages that are not run left out."""
    out = []
    for kind, i, val in (COMMANDS if commands is None else commands).get(k, []):
        if kind == "rx_set":
            out.append((kind, i, val))
        elif kind in stages:
            prm[kind][i] = val
            out.append((kind, i, val))
    return out


def oracle_channel(orc, sig, i, taps=TAPS, nstep=NSTEP, stages=ALL_STAGES, cfm_sets=None, commands=None):
    """Channel i on the oracle alone through the whole scenario: the schedule rule with orc_sdracquisition when a search
    is due, orc_sdrthread_step for up to MAX_PERIODS periods per step while TRACK, the three restatements over each
    step's rows with the states carried, the detector's decision poked into the oracle -- flagsync = 1, synci -- at the
    next tracked step's start, and the host's commands.  sig: the recording of the channel's ring.  Returns
    dict(steps=[per step: state, attempts, losses, next_try, searched, flagacq, ndone, cnt, lost_word, lock / bsync /
    cfm = state copies, applied, loop=(flagsync, synci)], lost=[(step, cnt, reason)], handover=[(step, buffloc)],
    decided=[(step, synci, true synci)], cfm_events=[window events], bsync_events=[tests])."""
    name, ring, ctype, prn = CH[i][:4]
    L = orc.lib()
    ntap = 1 + 2 * taps["corrn"]
    oring = orc.make_ring(sig, sig.shape[0], 0)
    mk = lambda: orc.make_chan(prn, ctype=ctype, dtype=2, f_sf=RINGS[ring]["f_sf"], f_if=0.0, **taps)
    box = dict(o=mk(), b=C.c_uint64(0), pending=None, flagacq=0)
    assert (box["o"].rate, box["o"].nsamp) == (RATES[i], RINGS[ring]["nsamp"])
    prm = initial_prm(stages, cfm_sets)
    ch = dict(state=CH_SEARCH, next_try=first_try(ring), attempts=0, losses=0)
    st = dict(lock=lr.zero_state(), bsync=br.zero_state(), cfm=cr.zero_state())
    zero = dict(lock=lr.zero_state, bsync=br.zero_state, cfm=cr.zero_state)
    out = dict(steps=[], lost=[], handover=[], decided=[], cfm_events=[], bsync_events=[])
    applied, lost_word = 0, 0
    for k, wps in enumerate(wrpos(nstep)):
        wp = wps[ring - 1]
        for kind, j, val in apply_commands(prm, k, stages, commands):
            if j != i:
                continue
            if kind == "rx_set":
                ch["state"] = val
                if val == CH_SEARCH:
                    ch["next_try"] = wrpos(nstep)[k - 1][ring - 1]      # the ring's write position at the call
            else:
                st[kind] = zero[kind]()                                 # a set zeroes the named channels' states

        def search(w):
            o = box["o"] = mk()                                         # the hand-over leaves a fresh channel (cnt = 0)
            loc, _ = rc.oracle_search(orc, o, oring, w)
            box["b"], box["pending"], box["flagacq"] = C.c_uint64(loc), None, int(o.flagacq)
            if o.flagacq:
                out["handover"].append((k, loc))
            return bool(o.flagacq)

        searched = schedule_step(ch, wp, lost_word, search, ring)
        lost_word = 0
        o = box["o"]
        II, QQ, fs, nb = [], [], [], []
        cnt0 = int(o.cnt)
        if ch["state"] == CH_TRACK:
            if box["pending"] is not None:
                o.flagsync, o.synci = 1, box["pending"]
                box["pending"] = None
            oring.wrpos = wp
            while len(fs) < MAX_PERIODS and L.orc_sdrthread_step(C.byref(o), C.byref(oring), C.byref(box["b"])):
                II.append(np.ctypeslib.as_array(o.II)[:ntap].copy())
                QQ.append(np.ctypeslib.as_array(o.QQ)[:ntap].copy())
                fs.append(int(o.flagsync))
                nb.append(int(o.bit) if (o.flagsync and o.swsync) else 0)
        nd = len(fs)
        if nd:
            II, QQ = np.array(II), np.array(QQ)
            if prm["bsync"][i] is not None:
                was = st["bsync"]["done"]
                br.run(st["bsync"], prm["bsync"][i], RATES[i], II[:, 0], QQ[:, 0], fs, nd, cnt0, events=out["bsync_events"])
                if st["bsync"]["done"] == 1 and was == 0:
                    out["decided"].append((k, st["bsync"]["synci"], true_synci(i, out["handover"][-1][1])))
                    if not o.flagsync:                                  # the preset, seen by the next step's first period
                        box["pending"] = st["bsync"]["synci"]
                        applied += 1
            if prm["lock"][i] is not None:
                ev = []
                lr.run(st["lock"], prm["lock"][i], RATES[i], II[:, 0], QQ[:, 0], fs, nb, nd, cnt0, events=ev)
                for e in ev:
                    if e[0] == "lost":
                        lost_word = 1
                        out["lost"].append((k, e[1], e[2]))
            if prm["cfm"][i] is not None:
                cr.run(st["cfm"], cr.prm(**prm["cfm"][i]), RATES[i], taps["corrn"], II, QQ, fs, nb, nd, cnt0, events=out["cfm_events"])
        preset = box["pending"] is not None
        out["steps"].append(dict(state=ch["state"], attempts=ch["attempts"], losses=ch["losses"], next_try=ch["next_try"],
                                 searched=searched, flagacq=box["flagacq"], ndone=nd, cnt=int(o.cnt), lost_word=lost_word,
                                 lock=dict(st["lock"]), bsync=br.copy_state(st["bsync"]), cfm=cr.copy_state(st["cfm"]),
                                 applied=applied, loop=(1 if preset else int(o.flagsync), box["pending"] if preset else int(o.synci))))
    return out
