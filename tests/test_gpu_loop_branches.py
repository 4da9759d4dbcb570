"""The closed loop on the device at the branches and cadences no synthetic signal reaches (tests/loop_branch_cases.py;
tests/test_loop_branch_host.py proves on the CPU, with the oracle alone, that every row reaches its branch).

* Filter branches: the rows of the filter table as channels of one engine on a ring of zeros, one period each.  The
  NaN rows (0/0 in the DLL) are the last period of their run: nothing is planned from them, and the engine is closed
  without another run -- no period on the device ever starts from a non-finite frequency.
* Vote synchronisation, bit decision and filter cadences: one channel per table row on seeded noise, 130 periods in two
  runs split inside an interval, every period against orc_sdrthread_step (tests/test_gpu_loop.py::_check_against_oracle).

Bounds.  Sums, sample counts, flags, remainders, nav state: exact.  Filter outputs on the zero ring: the project's 1e-14
(_close) against the oracle and against the mpmath restatement, the exact values (+-0.5, -1, 0, +-1, pi/2, NaN) equal
outright.  Filter outputs on noise: 1e-12, the bound of test_closed_loop_random_states_across_front_ends for the same
kind of run (the loops wander on noise, and one ulp of atan / atan2 is multiplied by the loop gains)."""
import ctypes as C
import math

import numpy as np
import pytest

import loop_branch_cases as lc
from test_gpu_loop import _check_against_oracle, _close

pytestmark = pytest.mark.gpu
LOG_FILTER = ("carrErr", "codeErr", "freqErr", "carrNco", "codeNco")


def _nan_close(a, b, tol=1e-14):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return _close(a, b, tol)


# ---- filter branches ------------------------------------------------------------------------------------------------
def _filter_case(gc, orc, engine, capsys, dtype, f_if, taps):
    rows = lc.FILTER_ROWS
    ntap = 1 + 2 * taps[0]
    chans = [gc.Channel(6 + i, dtype=dtype, f_if=f_if, corrn=taps[0], corrd=taps[1], corrp=taps[2]) for i in range(len(rows))]
    n = 16368 * 3
    data = lc.make_ring_data("zero", dtype, n)
    engine.ring_create(1, dtype, n)
    engine.ring_push_raw(1, data, n)
    engine.set_channels(chans)
    ring = orc.make_ring(data, n, n)
    ochs, states, loops, restated = [], [], [], []
    for i, (row, c) in enumerate(zip(rows, chans)):
        o = lc.filter_oracle_chan(orc, row, i, taps, dtype, f_if)
        assert (o.ne, o.nl) == (c.ne, c.nl) == ((3, 4) if ntap == 13 else (1, 2))
        st = lc.filter_start(i, f_if, c.crate)
        ls = engine.loop_state(i, o.acq.acqfreq, flagsync=0, synci=0, cnt=0)
        lc.apply_presets(ls, lc.filter_presets(row, c.ne, c.nl))
        restated.append(lc.restate_row(row, o, 0, o.ctime, through_step=True))
        ochs.append(o)
        states.append(st)
        loops.append(ls)
    engine.trk_set_state(states)
    engine.loop_set(loops)
    engine.trk_run_loop(1)                              # the only run of this engine: the NaN rows end it
    II, QQ, ns = engine.trk_fetch()
    log, ndone = engine.trk_fetch_log()
    fin = engine.trk_get_state()
    lst = engine.loop_get()
    assert np.all(ndone == 1)
    lines = []
    for i, (row, o) in enumerate(zip(rows, ochs)):
        name = row["name"]
        b = C.c_uint64(states[i]["buffloc"])
        assert orc.lib().orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(b)) == 1
        r = log[i, 0]
        # the period itself: bit for bit
        assert not np.any(II[i, 0]) and not np.any(QQ[i, 0]), name
        assert not any(o.II[t] or o.QQ[t] for t in range(ntap)), name
        assert ns[i, 0] == o.currnsamp == r["currnsamp"] and 16000 < o.currnsamp < 16400, name
        assert r["remcode"] == o.remcode and r["remcarr"] == o.remcarr, name
        assert r["flagloopfilter"] == o.flagloopfilter == 1 and r["flagsync"] == 0 and r["navbit"] == 0, name
        assert fin[i]["buffloc"] == b.value and fin[i]["remcode"] == o.remcode and fin[i]["remcarr"] == o.remcarr, name
        assert lst[i].cnt == o.cnt == 1 and lst[i].flagsync == 0, name
        for f in ("sumI", "sumQ", "oldsumI", "oldsumQ", "II", "QQ"):               # cleared after the update
            assert np.array_equal(np.ctypeslib.as_array(getattr(lst[i], f))[:ntap],
                                  np.ctypeslib.as_array(getattr(o, f))[:ntap]), (name, f)
            assert not np.any(np.ctypeslib.as_array(getattr(lst[i], f))[:ntap]), (name, f)
        # the device's own values agree with each other exactly
        dev = dict(carrfreq=float(r["carrfreq"]), codefreq=float(r["codefreq"]))
        for f in ("carrfreq", "codefreq"):
            assert lc.same_double(fin[i][f], dev[f]), (name, f, fin[i][f], dev[f])
        for f in LOG_FILTER:
            dev[f] = float(r[f])
            assert lc.same_double(getattr(lst[i], f), dev[f]), (name, f, getattr(lst[i], f), dev[f])
        # against the oracle: 1e-14, NaN where NaN; the exact values outright
        for f in ("carrfreq", "codefreq") + LOG_FILTER:
            assert _nan_close(dev[f], getattr(o, f)), (name, f, dev[f], getattr(o, f))
        for f, v in lc.exact_outputs(row, through_step=True).items():
            assert lc.same_double(dev[f], v) and lc.same_double(getattr(o, f), v), (name, f, dev[f], getattr(o, f), v)
        nan_row = row["branch"].get("dll") == "0/0"
        assert math.isnan(dev["codefreq"]) == math.isnan(dev["codeNco"]) == math.isnan(dev["codeErr"]) == nan_row, name
        assert math.isfinite(dev["carrfreq"]), name
        # against the restatement: the same bound (a row beyond it on the device alone would be a finding)
        p, dll_of = restated[i]
        d = dll_of(dev["carrfreq"])
        want = {f: (p if f in p else d)[f] for f in ("carrfreq", "codefreq") + LOG_FILTER}
        for f, w in want.items():
            if isinstance(w, float) and math.isnan(w):
                assert math.isnan(dev[f]), (name, f)
            else:
                assert _close(dev[f], float(w)), (name, f, dev[f], float(w))
        lines.append("%-28s " % name + " ".join("%s %.2f/%.2f" % (f, lc.ulps_from(dev[f], want[f]), lc.ulps_from(getattr(o, f), want[f]))
                                                 for f in want))
    with capsys.disabled():
        print("\nulps from the restatement, device/oracle, prm1, %d taps, dtype %d:" % (ntap, dtype))
        print("\n".join(lines))


def test_filter_branches_iq_13_taps(gc, orc, engine, capsys):
    """Every row of the filter table, int8 IQ at zero IF, the 13-tap layout (early / late at taps 3 / 4)."""
    _filter_case(gc, orc, engine, capsys, 2, 0.0, (6, 3, 6))


def test_filter_branches_real_if_5_taps(gc, orc, engine, capsys):
    """Every row of the filter table, real samples at a 4.092 MHz IF, 5 taps (early / late at taps 1 / 2)."""
    _filter_case(gc, orc, engine, capsys, 1, 4.092e6, (2, 3, 3))


# ---- vote sync, bit decision, cadences on noise -----------------------------------------------------------------------
def _oracle_obs_rows(orc, o, ring, buffloc, rows):
    """The oracle's setobsdata() rows over the periods of `rows` (the device's log of one run) for the clone `o` of a
    channel's oracle state before that run: stepped and handed the device's filter outputs exactly as _adopt does."""
    from test_gpu_loop import FILTER_FIELDS
    want = []
    for r in rows:
        nobs = o.obs_n
        assert orc.lib().orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(buffloc)) == 1
        if o.obs_n != nobs:
            want.append((o.obs_tow, o.obs_remcout, o.obs_L, o.obs_D, o.obs_S, o.obs_Isum == 0.0, o.obs_codei, o.obs_cntout))
        for f in FILTER_FIELDS:
            setattr(o, f, float(r[f]))
    return want


def _noise_case(gc, orc, engine, rows, kmax):
    F = lc.NAV_FRONT
    taps = F["taps"]
    ntap = 1 + 2 * taps[0]
    chans = [gc.Channel(r["prn"], dtype=F["dtype"], f_sf=F["f_sf"], f_if=F["f_if"], corrn=taps[0], corrd=taps[1], corrp=taps[2])
             for r in rows]
    nsamp = chans[0].nsamp
    assert nsamp == 4092 and max(min(r["presets"]["loopms"], 20) for r in rows) == kmax
    n = nsamp * (lc.NAV_NPER + 4)
    data = lc.make_ring_data("noise", F["dtype"], n, lc.NAV_SEED)
    engine.ring_create(1, F["dtype"], n)
    engine.ring_push_raw(1, data, n)
    engine.set_channels(chans)
    ring = orc.make_ring(data, n, n)
    ochs, bufflocs, states, loops, obs = [], [], [], [], {}
    for i, (row, c) in enumerate(zip(rows, chans)):
        st = lc.start_state(row["st"], F["f_if"], c.crate, nsamp, lc.NAV_SEED)
        o = lc.oracle_chan(orc, row, st, F["dtype"], F["f_sf"], F["f_if"], taps)
        ls = engine.loop_state(i, o.acq.acqfreq)
        lc.apply_presets(ls, row["presets"])
        ochs.append(o)
        bufflocs.append(C.c_uint64(st["buffloc"]))
        states.append(st)
        loops.append(ls)
        if row["name"] in lc.OBS_ROWS:
            s = gc.ObsState()
            s.f_sf, s.f_if, s.foffset, s.ctime, s.loopms = o.f_sf, o.f_if, o.foffset, o.ctime, o.loopms
            s.oldremcode = o.remcode
            obs[i] = s
            assert 100 // o.loopms == {3: 33, 20: 5}[o.loopms]
    engine.trk_set_state(states)
    engine.loop_set(loops)
    done, logs = 0, []
    for nrun in lc.NAV_CHUNKS:
        clones = {i: (type(ochs[i]).from_buffer_copy(ochs[i]), C.c_uint64(bufflocs[i].value), ochs[i].cnt) for i in obs}
        _check_against_oracle(orc, engine, ochs, ring, bufflocs, nrun, ntap, done=done, tol=1e-12)
        II, _, _ = engine.trk_fetch()
        log, _ = engine.trk_fetch_log()
        logs.append(log)
        for i, (clone, b, cnt0) in clones.items():       # setobsdata over the device's log (as test_gpu_loop.py::_run_case)
            want = _oracle_obs_rows(orc, clone, ring, b, log[i])
            got = gc.obs_replay(obs[i], log[i], II[i, :, 0], cnt0=cnt0)
            assert len(got) == len(want) > 0, (rows[i]["name"], len(got), len(want))
            for r, w in zip(got, want):
                assert r["tow"] == w[0] and int(r["codei"]) == w[6] and int(r["cntout"]) == w[7], (rows[i]["name"], w)
                assert _close(r["remcout"], w[1]) and _close(r["L"], w[2], 1e-12) and _close(r["D"], w[3]), (rows[i]["name"], w)
                assert bool(r["snr"]) == w[5] and (not w[5] or _close(r["S"], w[4], 1e-12)), (rows[i]["name"], w)
        done += nrun
    log = np.concatenate(logs, axis=1)
    fin = engine.trk_get_state()
    lst = engine.loop_get()
    bits = {}
    for i, (row, o) in enumerate(zip(rows, ochs)):
        name, x = row["name"], row["expect"]
        assert fin[i]["buffloc"] == bufflocs[i].value and fin[i]["remcode"] == o.remcode and fin[i]["remcarr"] == o.remcarr, name
        assert o.flagsync == 1 and lst[i].flagsync == 1, name
        for f in ("synci", "biti", "navcnt", "swloop", "bit", "swsync", "swreset", "bitIP", "cnt", "flagpol", "rate", "loopms"):
            assert getattr(lst[i], f) == getattr(o, f), (name, f, getattr(lst[i], f), getattr(o, f))
        assert list(lst[i].bitsync) == list(o.bitsync), name
        assert lst[i].cnt == row["presets"]["cnt"] + lc.NAV_NPER, name
        # in the log: the period of flagsync, the decided bits, the filter updates -- as the host test found them
        fs = log[i]["flagsync"]
        first = int(np.argmax(fs != 0))
        assert first == x["sync"] and np.all(fs[first:] == 1) and not np.any(fs[:first]), (name, first)
        assert np.all(log[i]["flagloopfilter"][:first] == 1), name
        upd = np.flatnonzero(log[i]["flagloopfilter"] == 2)
        assert set(int(g) for g in np.diff(upd)) == x["gaps"] and len(upd) == x["nupd"], (name, upd)
        assert (int(upd[0]) if len(upd) else None) == x["first"], name
        assert set(np.unique(log[i]["flagloopfilter"][first:])) <= {0, 2}, name
        bits[name] = [int(v) for v in log[i]["navbit"] if v]
        assert len(bits[name]) == x["nbits"], (name, len(bits[name]))
        if x["sync"] > 0:
            assert lst[i].synci == x["synci"], name
    return bits


def test_vote_sync_and_bit_decision(gc, orc, engine):
    """The vote path of checksync() (PRN 1-5: bin 0 with the wrap of synci to rate - 1, a middle bin, two bins with the
    later one hit, cnt crossing 2^32 before the vote falls, rates 20 / 10 / 2) and the rate-1 shortcut, then checkbit()'s
    decisions under flagpol 0 and 1 and the filter cadence from the bit edge found."""
    bits = _noise_case(gc, orc, engine, lc.NAV_ROWS, kmax=10)
    a, b = (bits[n] for n in lc.FLAGPOL_PAIR)
    assert a == [-v for v in b] and set(a) == {1, -1}


def test_cadences_side_by_side(gc, orc, engine):
    """loopms 1, 2, 3, 7, 10, 20, 25 against rates 20, 10, 2, 1 in one engine: the step's capacity is GC_STEP_KMAX = 20 (a
    full 20-period interval; loopms 25 cut there with no filter at its end) and each channel's interval is its own."""
    _noise_case(gc, orc, engine, lc.CADENCE_ROWS, kmax=20)


def test_cadences_largest_loopms_3(gc, orc, engine):
    """An engine whose step holds three periods: loopms 1, 2, 3 against every rate."""
    _noise_case(gc, orc, engine, [r for r in lc.CADENCE_ROWS if r["presets"]["loopms"] <= 3], kmax=3)


def test_cadences_cnt_around_2_32(gc, orc, engine):
    """cnt crossing 2^32 inside the run and cnt far above it: nav_biti's 64-bit remainder (2^32 mod 20 = 16)."""
    _noise_case(gc, orc, engine, lc.CNT_ROWS, kmax=7)
