"""Lock monitor (gnsscorr_lock_run, gnsscorr_rx_lock_set, gnsscorr_rx_lock_status), the part that needs no GPU: the ABI,
the restated detector (tests/lock_restate.py) on streams whose answers are known by hand, and -- on the CPU oracle
alone -- that the scenario of tests/test_gpu_rx_lock.py decides what it is meant to decide."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import fec_restate as fr
import lock_cases as lc
import lock_restate as lr
import lock_sbas_cases as ls
import sbas_if_cases as sic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gnsscorr_lock_run", "gnsscorr_rx_lock_set", "gnsscorr_rx_lock_status"]


def test_lock_symbols_exported_and_declared(gc):
    L = gc.lib()
    hdr = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    for name in NEW_SYMBOLS:
        getattr(L, name)
        assert name in gc.EXPORTS_GNSSCORR and (name + "(") in hdr.replace(" (", "("), name
    assert '"rx_lock"' in hdr


def _layout(tmp_path, ctype_name, fields):
    src = tmp_path / ("sz_%s.c" % ctype_name)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gnsscorr.h"\nint main(){printf("%%zu", sizeof(%s));\n' % ctype_name +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (ctype_name, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / ("sz_%s" % ctype_name)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(v) for v in subprocess.check_output([str(exe)]).split()]


def test_lock_struct_layouts(gc, tmp_path):
    """sizeof/offsetof of gnsscorr_lockprm_t and gnsscorr_lock_t compiled from include/gnsscorr.h against the ctypes
    mirrors; gnsscorr_rxstat_t keeps its size."""
    f = ["sync_periods", "kbits", "nbad", "pad", "mu_min"]
    vals = _layout(tmp_path, "gnsscorr_lockprm_t", f)
    assert vals[0] == C.sizeof(gc.LockPrm) == 24
    assert vals[1:] == [getattr(gc.LockPrm, n).offset for n in f] == [0, 4, 8, 12, 16]
    f = list(lr.FIELDS)
    vals = _layout(tmp_path, "gnsscorr_lock_t", f)
    assert vals[0] == C.sizeof(gc.LockState) == 80
    assert vals[1:] == [getattr(gc.LockState, n).offset for n in f] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 68, 72, 76]
    assert [n for n, _ in gc.LockState._fields_] == f
    assert _layout(tmp_path, "gnsscorr_rxstat_t", ["cnt"]) == [80, 72]


def test_lock_calls_fail_loudly_without_a_context(gc):
    L = gc.lib()
    prm = gc.LockPrm(0, 10, 2, 0, 5.0)
    st = (gc.LockState * 1)()
    one = (C.c_int * 1)(0)
    buf = C.addressof(st)
    assert L.gnsscorr_lock_run(None, buf, buf, buf, buf, buf, buf, buf, buf, 1, 1) == -1
    assert b"null" in L.gnsscorr_last_error()
    assert L.gnsscorr_rx_lock_set(None, 0, 1, C.byref(prm)) == -3
    assert b"rx_start" in L.gnsscorr_last_error()
    assert L.gnsscorr_rx_lock_status(None, st, one) == -3
    assert bytes(st) == bytes(C.sizeof(st))


# ---- the restatement on streams with answers known by hand --------------------------------------------------------------
def _bits(n, rate, phase):
    """navbit column: a decided bit in every period e with e % rate == phase."""
    nb = np.zeros(n, np.int32)
    nb[phase::rate] = 1
    return nb


def _run(prm, rate, I, Q, fs, nb, cnt0=5, st=None):
    ev = []
    st = lr.run(lr.zero_state() if st is None else st, prm, rate, I, Q, fs, nb, len(I), cnt0, events=ev)
    return st, ev


@pytest.mark.parametrize("rate", [20, 10, 2])
def test_restatement_constant_signal_gives_np_equal_rate(rate):
    n = 12 * rate
    prm = dict(sync_periods=0, kbits=4, nbad=2, mu_min=1.5)
    st, ev = _run(prm, rate, np.ones(n), np.zeros(n), np.ones(n, np.int32), _bits(n, rate, 1))
    nps = [e[2] for e in ev if e[0] == "np"]
    assert len(nps) == 11 and all(v == float(rate) for v in nps)        # the bit before the first edge is not whole
    mus = [e for e in ev if e[0] == "mu"]
    assert len(mus) == 2 and all(e[2] == float(rate) for e in mus)
    assert mus[0][1] == 5 + 1 + 4 * rate                                # cnt of the row that closed the fourth whole bit
    assert (st["windows"], st["k"], st["nbad"], st["lost"], st["mu_last"]) == (2, 3, 0, 0, float(rate))
    assert st["npsum"] == 3.0 * rate and st["open"] == 1 and st["n"] == rate - 2 and st["sI"] == float(rate - 2)


def test_restatement_alternating_signs_and_zero_rows():
    rate, n = 20, 200
    prm = dict(sync_periods=0, kbits=2, nbad=3, mu_min=1.0)
    alt = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    st, ev = _run(prm, rate, alt, -alt, np.ones(n, np.int32), _bits(n, rate, 0))
    assert [e[2] for e in ev if e[0] == "np"] == [0.0] * 6             # nothing is read behind the loss
    assert [e for e in ev if e[0] == "lost"] == [("lost", 5 + 120, 2)]  # windows end at bits 2, 4, 6: rows 40, 80, 120
    assert (st["lost"], st["reason"], st["lost_cnt"], st["windows"], st["nbad"]) == (1, 2, 125, 3, 3)
    assert (st["open"], st["n"], st["sI"], st["sQ"], st["w"], st["k"], st["npsum"]) == (1, 0, 0.0, 0.0, 0.0, 0, 0.0)
    # all-zero rows: w is not > 0, so np = 0.0 and not a division by zero
    st, ev = _run(prm, rate, np.zeros(n), np.zeros(n), np.ones(n, np.int32), _bits(n, rate, 0))
    assert [e[2] for e in ev if e[0] == "np"][:6] == [0.0] * 6 and st["lost"] == 1 and st["lost_cnt"] == 125
    assert not math.isnan(st["mu_last"]) and st["mu_last"] == 0.0


def test_restatement_drops_a_bit_of_seven_periods():
    rate, n = 20, 140
    nb = _bits(n, rate, 10)                                              # edges at 10, 30, 50, ...
    nb[37] = -1                                                          # a bit of 7 periods, then one of 13
    prm = dict(sync_periods=0, kbits=1, nbad=100, mu_min=1.0)
    st, ev = _run(prm, rate, np.ones(n), np.zeros(n), np.ones(n, np.int32), nb)
    assert [e[1] - 5 for e in ev if e[0] == "np"] == [30, 70, 90, 110, 130]   # neither 37 nor 50 closed a whole bit
    assert all(e[2] == 20.0 for e in ev if e[0] == "np") and st["windows"] == 5


def test_restatement_timeout_fires_exactly_at_sync_periods():
    n = 50
    prm = dict(sync_periods=40, kbits=10, nbad=2, mu_min=5.0)
    z = np.zeros(n)
    st, ev = _run(prm, 20, z, z, np.zeros(n, np.int32), np.zeros(n, np.int32), cnt0=5)
    assert ev == [("lost", 39, 1)] and (st["lost"], st["reason"], st["lost_cnt"]) == (1, 1, 39)   # cnt + 1 == 40
    st, ev = _run(prm, 20, z[:34], z[:34], np.zeros(34, np.int32), np.zeros(34, np.int32), cnt0=5)
    assert ev == [] and st["lost"] == 0                                  # the last row has cnt + 1 == 39
    # synchronised in time: no timeout, and none later either
    fs = np.zeros(n, np.int32)
    fs[34:] = 1
    st, ev = _run(prm, 20, z, z, fs, np.zeros(n, np.int32), cnt0=5)
    assert ev == [] and st["lost"] == 0
    # sync_periods 0: no such rule; cnt0 == 0 resets a lost state, any other cnt0 keeps it frozen
    st, ev = _run(dict(prm, sync_periods=0), 20, z, z, np.zeros(n, np.int32), np.zeros(n, np.int32), cnt0=5)
    assert ev == [] and st["lost"] == 0
    lost = dict(lr.zero_state(), lost=1, reason=2, lost_cnt=77, sI=3.0, n=4, open=1)
    st, ev = _run(prm, 20, np.ones(n), z, np.ones(n, np.int32), _bits(n, 20, 0), cnt0=1, st=dict(lost))
    assert st == lost and ev == []
    st, ev = _run(prm, 20, np.ones(n), z, np.ones(n, np.int32), _bits(n, 20, 0), cnt0=0, st=dict(lost))
    assert st["lost"] == 0 and st["lost_cnt"] == 0 and st["k"] == 2 and st["npsum"] == 40.0


def test_restatement_threshold_is_strict():
    """mu == mu_min is not bad; mu_min one ulp above mu is."""
    rate, n = 20, 100
    rng = np.random.default_rng(3)
    I = rng.integers(-2 ** 20, 2 ** 20, n) / 32.0
    Q = rng.integers(-2 ** 20, 2 ** 20, n) / 32.0
    prm = dict(sync_periods=0, kbits=2, nbad=1, mu_min=1e-9)
    _, ev = _run(prm, rate, I, Q, np.ones(n, np.int32), _bits(n, rate, 0))
    mu = [e[2] for e in ev if e[0] == "mu"][0]
    assert 0.0 < mu < 20.0
    st, ev = _run(dict(prm, mu_min=mu), rate, I, Q, np.ones(n, np.int32), _bits(n, rate, 0))
    assert ev[2][0] == "mu" and ev[2][2] == mu and not any(e[0] == "lost" for e in ev[:3]) and st["windows"] == 2
    st, ev = _run(dict(prm, mu_min=float(np.nextafter(mu, np.inf))), rate, I, Q, np.ones(n, np.int32), _bits(n, rate, 0))
    assert ev[3] == ("lost", 5 + 40, 2) and st["windows"] == 1 and st["nbad"] == 1


def test_mu_from_cn0_closed_form(gc):
    for cn0, rate, ctime in ((47.0, 20, 1e-3), (30.0, 10, 1e-3), (38.5, 2, 1e-3), (25.0, 20, 1e-3)):
        x = 10.0 ** (cn0 / 10.0) * ctime
        mu = gc.mu_from_cn0(cn0, rate, ctime)
        assert mu == (1.0 + rate * x) / (1.0 + x) and 1.0 < mu < rate
        # the inverse: C/N0 = (mu - 1) / ((rate - mu) * ctime)
        assert abs(10.0 * math.log10((mu - 1.0) / ((rate - mu) * ctime)) - cn0) < 1e-9
    assert gc.mu_from_cn0(-300.0, 20, 1e-3) == 1.0 and abs(gc.mu_from_cn0(300.0, 20, 1e-3) - 20.0) < 1e-12


# ---- the scenario, on the oracle alone -----------------------------------------------------------------------------
def test_loss_of_lock_scenario_is_decided_by_the_oracle(gc, orc, synth):
    """The oracle free-running through the schedule rule and the restated detector: PRN 5 synchronises late (the
    vote-histogram branch) and is never lost, PRN 12 is lost by the power rule within (nbad + 1) * kbits * rate periods
    of its switch-off, fails its re-search in the gap and is acquired again after the signal has returned, PRN 30 never
    synchronises and is lost by the time limit, PRN 9 fails every search.  Conditions on the input (seed, C/N0, switch
    times), not tolerances: a device run that lost nothing, or everything, could not agree with them."""
    sig = lc.signal(gc, synth)
    assert sig.shape == (lc.NCHUNK * lc.CHUNK, 2) and lc.NCHUNK == 32 and lc.CHUNK == 250 * lc.NSAMP
    H = {p: lc.oracle_schedule(gc, orc, sig, p, lc.prm_of(p)) for p in lc.PRNS}
    mus = lambda h: [(e[1], e[2], e[3]) for e in h["events"] if e[0] == "mu"]
    lost = lambda h: [(e[1], e[2], e[3]) for e in h["events"] if e[0] == "lost"]
    states = lambda h: [s["state"] for s in h["steps"]]
    searches = lambda h: [(k, s["flagacq"]) for k, s in enumerate(h["steps"]) if s["searched"]]

    h = H[5]
    assert searches(h) == [(0, 1)] and states(h) == [2] * 32 and h["steps"][-1]["losses"] == 0
    assert h["sync"] == [4040] and 2600 < 4040 < 6000                   # PRM's time limit would have cut it off
    assert len(mus(h)) == 18 and min(m[2] for m in mus(h)) >= 19.0 and lost(h) == []

    h = H[12]
    assert h["sync"] == [2020, 2039] and h["runs"] == 2
    m = mus(h)
    assert [x[1] for x in m[:6]] == [2220, 2420, 2620, 2820, 3020, 3220]
    assert all(x[2] > 16.5 for x in m[:3]) and 5.0 < m[3][2] < 16.5 and m[4][2] < 2.0 and m[5][2] < 2.0
    assert lost(h) == [(13, 3220, 2)]
    limit = (lc.PRM["nbad"] + 1) * lc.PRM["kbits"] * lc.RATE * 1e-3     # seconds
    assert len(h["lost_t"]) == 1 and lc.T_OFF_12 < h["lost_t"][0] <= lc.T_OFF_12 + limit
    # lost in step 13, searched in step 14 in the gap (fails), paused 1.5 s, acquired in step 20 (5.25 s)
    assert searches(h) == [(0, 1), (14, 0), (20, 1)]
    assert h["steps"][14]["peakr"] < 1.6 and h["steps"][20]["peakr"] > gc.ACQTH + 0.3
    assert states(h) == [2] * 14 + [1] * 6 + [2] * 12
    assert [s["losses"] for s in h["steps"]] == [0] * 14 + [1] * 18
    assert h["steps"][20]["cnt"] == h["steps"][20]["ndone"] < lc.MAX_PERIODS       # cnt restarted
    assert all(x[2] > 16.5 for x in m[6:]) and len(m) == 9

    h = H[30]
    assert searches(h)[0] == (0, 1) and h["steps"][0]["peakr"] > gc.ACQTH + 0.3
    assert h["sync"] == [None] and mus(h) == [] and lost(h) == [(11, 2599, 1)]
    assert states(h) == [2] * 12 + [1] * 20 and h["steps"][-1]["losses"] == 1
    assert [f for _, f in searches(h)[1:]] == [0] * 4 and [k for k, _ in searches(h)] == [0, 12, 18, 24, 30]

    h = H[9]
    assert [f for _, f in searches(h)] == [0] * 6 and states(h) == [1] * 32 and lost(h) == []
    assert all(s["peakr"] < 2.0 for s in h["steps"] if s["searched"])


# ---- rate 2: SBAS channels inside the schedule, on the oracle alone ---------------------------------------------------
def _windows(h, handover):
    """[(start s, end s, mu)] of the monitor's windows of one oracle_schedule history, on the stream's clock: a window that
    closes in the row with cnt c holds the KBITS symbols of the rows c - 2*KBITS + 1 .. c of the run that began at sample
    `handover`."""
    out = []
    for e in h["events"]:
        if e[0] == "mu":
            end = (handover + (e[2] + 1) * ls.NSAMP) / ls.F_SF
            out.append((end - 2 * ls.KBITS * 1e-3, end, e[3]))
    return out


def _replay(rows, run):
    """SbasReplay over the decided symbols of one hand-over's rows (oracle_schedule with keep_rows)."""
    sym, cnts, locs = [], [], []
    for r in rows:
        if r["run"] == run:
            k = np.flatnonzero(r["navbit"])
            sym += list(r["navbit"][k])
            cnts += list(r["cnt0"] + k)
            locs += list(r["buffloc"][k])
    return sic.replayed(sym, cnts, locs), np.array(cnts)


def test_rate2_thresholds_and_scenario_on_the_oracle(gc, orc, synth):
    """tests/lock_sbas_cases.py on the oracle alone, free-running.

    Thresholds.  With the detector watching only (nbad out of reach) the window means of KBITS = 50 symbols are measured:
    the smallest of a channel locked on the right edge (PRN 120 while it is on, PRN 133 after its second hand-over) and
    the largest of everything else (PRN 120's noise after T_OFF, PRN 133 on the wrong edge).  They are the numbers the
    case file and DESIGN.md 3.2b state, MU_MIN is their midpoint, and each keeps a quarter of the detector's whole
    range at rate 2 (1 to 2) from it: a window length that separates the two only barely fails here.

    Decisions.  PRN 120 finds the right edge as its hand-over predicts, is never lost while on, holds its frame at the
    predicted cnt and is lost by the power rule within NBAD + 1 windows of T_OFF; reason 1 never applies to an SBAS
    channel (it synchronises on the first two like signs behind cnt 2000, signal or not).  PRN 133 finds the wrong
    edge, looks like noise to the monitor, is lost by the power rule two windows later and searched again; its second
    hand-over starts one code period off the first one's parity, finds the right edge and stays -- too late for a frame
    in this recording.  PRN 12 (L1 C/A, the thresholds of tests/lock_cases.py) is never lost."""
    sig = ls.signal(gc, synth)
    assert sig.shape == (ls.NCHUNK * ls.CHUNK, 2) and ls.NCHUNK == 28 and ls.RATES == [2, 2, 20]
    W = [ls.oracle_schedule(gc, orc, sig, i, ls.PRM_WATCH) for i in (0, 1)]
    H = [ls.oracle_schedule(gc, orc, sig, i, keep_rows=True) for i in (0, 1, 2)]
    lost = lambda h: [(e[1], e[2], e[3]) for e in h["events"] if e[0] == "lost"]
    states = lambda h: [s["state"] for s in h["steps"]]
    searches = lambda h: [(k, s["flagacq"]) for k, s in enumerate(h["steps"]) if s["searched"]]
    limit = (ls.NBAD + 1) * ls.KBITS * 2 * 1e-3                          # seconds

    # ---- the thresholds
    assert W[0]["runs"] == W[1]["runs"] == 1 and lost(W[0]) == lost(W[1]) == []
    w0 = _windows(W[0], W[0]["handover"][0])
    on = [m for a, b, m in w0 if b <= ls.T_OFF]
    off = [m for a, b, m in w0 if a >= ls.T_OFF]
    assert len(on) == 40 and len(off) == 6 and len(w0) == 47            # one window straddles T_OFF
    assert H[1]["runs"] == 2 and ls.predict(1, H[1]["handover"][1])[2]
    relocked = [e[3] for e in H[1]["events"] if e[0] == "mu" and e[1] >= 10]      # (windows of the second run)
    wrong = [m for _, _, m in _windows(W[1], W[1]["handover"][0])]
    assert len(relocked) >= 20 and len(wrong) == 47
    lo, hi = min(on + relocked), max(off + wrong)
    print("rate 2, kbits %d: locked %.4f .. %.4f, noise %.4f .. %.4f, wrong edge %.4f .. %.4f" %
          (ls.KBITS, lo, max(on + relocked), min(off), max(off), min(wrong), max(wrong)))
    assert math.floor(lo * 100) / 100 == ls.MU_LOCKED_MIN and math.ceil(hi * 100) / 100 == ls.MU_OTHER_MAX
    assert ls.MU_MIN == 0.5 * (ls.MU_LOCKED_MIN + ls.MU_OTHER_MAX) and ls.PRM_SBAS["mu_min"] == ls.MU_MIN
    quarter = 0.25 * (ls.MU_LOCKED_MIN - ls.MU_OTHER_MAX)
    assert lo - ls.MU_MIN >= quarter and ls.MU_MIN - hi >= quarter       # (a quarter of the gap: true of any midpoint ...)
    assert lo - ls.MU_MIN >= 0.25 and ls.MU_MIN - hi >= 0.25             # ... and of the range 1 .. 2: true of a wide gap only

    # windows of 10 symbols, what the L1 C/A scenario uses, do not keep that distance on the same signal
    W10 = [ls.oracle_schedule(gc, orc, sig, i, dict(ls.PRM_WATCH, kbits=10)) for i in (0, 1)]
    w10 = [(a + 0.08, b, m) for a, b, m in _windows(W10[0], W10[0]["handover"][0])]        # (a window is 0.02 s long here)
    lo10 = min(m for a, b, m in w10 if b <= ls.T_OFF)
    hi10 = max([m for a, b, m in w10 if a >= ls.T_OFF] + [m for _, _, m in _windows(W10[1], 0)])
    print("rate 2, kbits 10: locked from %.4f, everything else up to %.4f" % (lo10, hi10))
    assert 1.9 < lo10 < lo and hi < hi10 < 1.6 and lo10 - hi10 < 0.5

    # ---- PRN 120: right edge, frame, loss after T_OFF
    h = H[0]
    row, synci, right, found = ls.predict(0, h["handover"][0])
    assert (row, synci, right, found) == (2002, 0, True, 5052)
    assert h["sync"] == [row] and h["runs"] == 1 and searches(h) == [(0, 1), (26, 0)]
    assert lost(h) == [(25, 6202, 2)] and len(h["lost_t"]) == 1 and ls.T_OFF < h["lost_t"][0] <= ls.T_OFF + limit
    assert states(h) == [2] * 26 + [1] * 2 and row + 1 < ls.PRM_SBAS["sync_periods"]
    rep, cnts = _replay(h["rows"], 1)
    assert np.all(np.diff(cnts) == 2) and cnts[0] == row
    assert (rep.flagdec, rep.firstsfcnt, rep.firstsftow, rep.week) == (1, found, ls.TOW, ls.WEEK)
    # 1000 periods behind the frame the next message is decoded: message 1 (type 2), one second later
    assert found + 1000 <= cnts[-1] < found + 2000 and (rep.id, rep.tow) == (2, ls.TOW + 1)
    assert rep.msg == bytes(np.packbits(np.array(sic.messages()[1] + [0] * 6, np.uint8))) and rep.polarity in (1, -1)

    # ---- PRN 133: wrong edge, lost as noise, searched again
    h = H[1]
    first, second = ls.predict(1, h["handover"][0]), ls.predict(1, h["handover"][1])
    assert first == (2002, 0, False, None) and second == (2003, 1, True, None)
    assert ls.code_period(1, h["handover"][0]) % 2 == 0 and ls.code_period(1, h["handover"][1]) % 2 == 0
    assert h["sync"] == [2002, 2003] and searches(h) == [(0, 1), (10, 1)]
    mus = [(e[1], e[2], e[3]) for e in h["events"] if e[0] == "mu"]
    assert [m[:2] for m in mus[:2]] == [(9, 2102), (9, 2202)] and all(m[2] < ls.MU_OTHER_MAX for m in mus[:2])
    assert lost(h) == [(9, 2202, 2)] and states(h) == [2] * 28 and [s["losses"] for s in h["steps"]] == [0] * 10 + [1] * 18
    assert all(m[2] > ls.MU_LOCKED_MIN for m in mus[2:])
    rep, cnts = _replay(h["rows"], 2)
    assert cnts[0] == 2003 and rep.flagtow == 0 and rep.fields() == fr.SbasReplay().fields()

    # ---- PRN 12 beside them
    h = H[2]
    assert searches(h) == [(0, 1)] and lost(h) == [] and states(h) == [2] * 28 and h["sync"] == [2039]
