"""gnsscorr_g1frame_replay on symbols, no GPU: the library against the literal restatement of tests/g1_restate.py, every
state field after every piece (everything here is exact: doubles compare with ==), and against what the streams of
tests/g1_strings.py were built to hold -- where the time mark is, what the strings say, the time by datetime arithmetic.
Memory safety: the stand-alone program tests/host/g1frame_host.c with csrc/sdr_g1.c alone under address and
undefined-behaviour sanitizers, run as a child process."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import g1_restate as gr
import g1_strings as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNT0, FIRST = 1234, 3                           # sdrthread's cnt at row 0; the row of the first symbol
DATE = (2023, 5, 17)                            # third year of interval 7
NT, N4 = gs.glonass_day(*DATE)
FIELDS = dict(tk=(14, 25, 1), nt=NT, n4=N4, slot=9, iode=33)
WEEK, TOW1 = gs.gps_week_tow(*DATE, 14, 25, 30)     # GPS time at which string 1 begins


def replay_both(gc, log, cnt0=CNT0, piece=2000, st=None, rep=None):
    """The library and the restatement over the same rows in pieces of `piece` rows, compared after every piece."""
    st = gc.G1FrameState() if st is None else st
    rep = gr.G1Replay() if rep is None else rep
    for a in range(0, len(log), piece):
        rows = log[a:a + piece]
        gc.g1frame_replay(st, rows, cnt0 + a)
        rep.run_log(rows["navbit"], rows["buffloc"], cnt0 + a)
        assert gr.state_fields(st) == rep.fields(), a
    return st, rep


def end_cnt(k, lead=0):
    """cnt of the row that decides the last symbol of the k-th string (0-based) behind `lead` symbols."""
    return CNT0 + FIRST + 10 * (lead + 200 * (k + 1) - 1)


def test_layout_and_errors(gc):
    assert (NT, N4, WEEK, TOW1) == (1233, 7, 2262, 300348)
    assert C.sizeof(gc.G1FrameState) == 912 and gc.G1FrameState.str.offset == 864 and gc.G1FrameState.firstsf.offset == 880
    L = gc.lib()
    st = gc.G1FrameState()
    C.memset(C.byref(st), 0x5a, C.sizeof(st))
    log = gs.log_rows(gc, [1, -1])
    assert L.gnsscorr_g1frame_replay(None, log.ctypes.data, 2, 0) == -1
    assert L.gnsscorr_g1frame_replay(C.byref(st), None, 2, 0) == -1
    assert L.gnsscorr_g1frame_replay(C.byref(st), log.ctypes.data, -1, 0) == -1
    assert bytes(st) == b"\x5a" * 912


# ---- the time mark ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("polarity", [1, -1])
@pytest.mark.parametrize("offset", [0, 1, 137, 171])
def test_time_mark_at_any_offset(gc, polarity, offset):
    """A mark behind `offset` symbols of meandered data (fewer than a string's 170: the unfilled history is zeros): found
    in the row of its last symbol with its polarity; the string decoded there says no time, so the flags drop."""
    sym = polarity * np.concatenate([gs.meandered_data(offset, 5), gr.MARK, gs.meandered_data(60, 6)])
    st, rep = replay_both(gc, gs.log_rows(gc, sym, FIRST, cnt0=CNT0), piece=10)
    cnt = CNT0 + FIRST + 10 * (offset + 29)
    assert rep.marks == [(cnt, polarity)]
    assert (st.firstsfcnt, st.firstsf, st.polarity, st.s1cnt) == (cnt, 1000 * cnt, polarity, 1)
    assert (st.flagsyncf, st.flagtow, st.flagdec, st.tow_gpst) == (0, 0, 0, 0.0)


def test_29_of_30_is_no_mark(gc):
    for k in range(30):
        mark = np.array(gr.MARK)
        mark[k] = -mark[k]
        sym = np.concatenate([gs.meandered_data(40, 7), mark, gs.meandered_data(40, 8)])
        st, rep = replay_both(gc, gs.log_rows(gc, sym, FIRST, cnt0=CNT0), piece=len(sym) * 10)
        assert rep.marks == [] and (st.firstsfcnt, st.s1cnt, st.flagsyncf, st.polarity) == (0, 0, 0, 0)


def test_meandered_data_never_matches(gc):
    """Runs of meandered data are at most 2 long and the mark opens with a run of 5: over 10^5 symbols no window of 30
    correlates to +-30, and the replay finds nothing."""
    sym = gs.meandered_data(100000, 11)
    runs = np.diff(np.flatnonzero(np.diff(sym)))
    assert runs.max() == 2
    corr = np.correlate(sym.astype(np.int64), np.array(gr.MARK, np.int64), "valid")
    assert np.abs(corr).max() < 30
    st, rep = replay_both(gc, gs.log_rows(gc, sym, 0, step=1), piece=25000)
    assert rep.marks == [] and (st.firstsfcnt, st.s1cnt, st.id) == (0, 0, 0)


def test_mark_while_flagtow_is_up_is_ignored(gc):
    sym, _ = gs.stream([1, 2, 3, 4, 5], 21, **FIELDS)
    extra = np.concatenate([gs.meandered_data(77, 9), gr.MARK, gs.meandered_data(170 - 107, 10), -np.array(gr.MARK)])
    st, rep = replay_both(gc, gs.log_rows(gc, np.concatenate([sym, extra]), FIRST, cnt0=CNT0))
    assert [m[0] for m in rep.marks] == [end_cnt(k) for k in range(5)]          # (four found and dropped, the fifth kept)
    assert (st.flagtow, st.flagdec, st.firstsfcnt, st.polarity) == (1, 1, end_cnt(4), 1)
    assert st.s1cnt == 6                        # the decode 2000 periods on still ran, on whatever the symbols were


# ---- string order, counters, flags -----------------------------------------------------------------------------------
def test_strings_1_to_5_merge_at_string_5(gc):
    sym, bits = gs.stream([1, 2, 3, 4, 5], 22, **FIELDS)
    st, rep = replay_both(gc, gs.log_rows(gc, sym, FIRST, cnt0=CNT0))
    assert (st.ephcnt, st.s1cnt, st.id, st.flagsyncf, st.flagtow, st.flagdec) == (5, 5, 5, 1, 1, 1)
    assert (st.week, st.tow_gpst, st.firstsftow) == (WEEK, TOW1 + 10.0, TOW1 + 10.0)
    assert (list(st.tk), st.nt, st.n4, st.slot, st.iode, st.update) == ([11, 25, 30], NT, N4, 9, 33, 1)
    assert (st.firstsfcnt, st.firstsf) == (end_cnt(4), 1000 * end_cnt(4)) and bytes(st.str) == gs.packed(bits[4])


def test_mid_frame_start_merges_at_string_2(gc):
    sym, bits = gs.stream([3, 4, 5, 1, 2], 23, polarity=-1, **FIELDS)
    st, rep = replay_both(gc, gs.log_rows(gc, sym, FIRST, cnt0=CNT0))
    assert (st.ephcnt, st.s1cnt, st.id, st.flagdec, st.polarity) == (5, 2, 2, 1, -1)
    assert (st.week, st.tow_gpst, st.firstsftow, st.firstsfcnt) == (WEEK, TOW1 + 4.0, TOW1 + 4.0, end_cnt(4))
    assert bytes(st.str) == gs.packed(bits[4])


def test_almanac_strings_alone_give_no_time(gc):
    sym, _ = gs.stream(list(range(6, 16)), 24, **FIELDS)
    log = gs.log_rows(gc, sym, FIRST, cnt0=CNT0)
    st, rep = gc.G1FrameState(), gr.G1Replay()
    for k in range(10):
        replay_both(gc, log[2000 * k:2000 * (k + 1)], CNT0 + 2000 * k, st=st, rep=rep)
        assert (st.flagsyncf, st.flagtow, st.flagdec, st.tow_gpst) == (0, 0, 0, 0.0)
        assert (st.id, st.s1cnt, st.ephcnt, st.firstsfcnt) == (6 + k, k + 1, 0, end_cnt(k))
    assert len(rep.marks) == 10


def test_other_ids_between_the_ephemeris_strings(gc):
    """Ids 0 and 6..15 count in s1cnt and not in ephcnt."""
    sym, _ = gs.stream([1, 0, 2, 6, 3, 15, 4, 9, 5], 25, **FIELDS)
    st, _ = replay_both(gc, gs.log_rows(gc, sym, FIRST, cnt0=CNT0))
    assert (st.ephcnt, st.s1cnt, st.flagdec) == (5, 9, 1) and st.tow_gpst == st.firstsftow == TOW1 + 18.0


def test_ephcnt_runs_past_5_without_a_second_merge(gc):
    """The time is merged while ephcnt is exactly 5: again at a string outside 1..5 that follows (s1cnt has moved on),
    never once the counter has passed 5 -- until the caller sets it back."""
    later = dict(FIELDS, tk=(20, 7, 0))
    week2, tow2 = gs.gps_week_tow(*DATE, 20, 7, 0)
    parts = [gs.stream([1, 2, 3, 4, 5, 6], 26, **FIELDS)[0], gs.stream([1, 2, 3, 4, 5], 27, **later)[0],
             gs.stream([1, 2, 3, 4, 5], 28, **later)[0]]
    log = gs.log_rows(gc, np.concatenate(parts), FIRST, cnt0=CNT0)
    st, rep = replay_both(gc, log[:10000])
    assert (st.ephcnt, st.tow_gpst, st.firstsftow) == (5, TOW1 + 10.0, TOW1 + 10.0)
    replay_both(gc, log[10000:12000], CNT0 + 10000, st=st, rep=rep)
    assert (st.id, st.ephcnt, st.s1cnt, st.tow_gpst, st.firstsftow) == (6, 5, 6, TOW1 + 12.0, TOW1 + 10.0)
    replay_both(gc, log[12000:22000], CNT0 + 12000, st=st, rep=rep)
    assert (st.ephcnt, st.s1cnt, list(st.tk), st.tow_gpst) == (10, 5, [17, 7, 0], TOW1 + 12.0)      # a stale time
    st.ephcnt = rep.ephcnt = 0                  # what the reference's syncthread does once it has the ephemeris
    replay_both(gc, log[22000:], CNT0 + 22000, st=st, rep=rep)
    assert (st.ephcnt, st.week, st.tow_gpst) == (5, week2, tow2 + 10.0)
    assert (st.flagtow, st.firstsfcnt, st.firstsftow) == (1, end_cnt(4), TOW1 + 10.0)               # the frame reference stays


def test_iode_change_sets_update(gc):
    log = gs.log_rows(gc, np.concatenate([gs.stream([2], 30 + i, iode=v)[0] for i, v in enumerate((0, 0, 37, 37))]), FIRST, cnt0=CNT0)
    st, rep = gc.G1FrameState(), gr.G1Replay()
    for k, want in enumerate([(0, 0), (0, 0), (37, 1), (37, 1)]):
        replay_both(gc, log[2000 * k:2000 * (k + 1)], CNT0 + 2000 * k, st=st, rep=rep)
        assert (st.iode, st.update) == want and st.ephcnt == k + 1


# ---- cuts ------------------------------------------------------------------------------------------------------------
def test_state_does_not_depend_on_the_cuts(gc):
    """Three strings (nine of ten rows decide no symbol), the log cut at every row; and row by row.  ephcnt preset to 2,
    as a caller may, so that the third string merges the time and raises flagdec."""
    sym, _ = gs.stream([4, 5, 1], 40, **FIELDS)
    log = gs.log_rows(gc, sym, FIRST, cnt0=CNT0, nper=6007)
    whole, rep = gc.G1FrameState(ephcnt=2), gr.G1Replay()
    rep.ephcnt = 2
    replay_both(gc, log, piece=len(log), st=whole, rep=rep)
    assert (whole.flagdec, whole.ephcnt, whole.s1cnt, whole.firstsfcnt, whole.tow_gpst) == (1, 5, 1, end_cnt(2), TOW1 + 2.0)
    want = bytes(whole)
    for cut in range(len(log) + 1):
        st = gc.G1FrameState(ephcnt=2)
        gc.g1frame_replay(st, log[:cut], CNT0)
        gc.g1frame_replay(st, log[cut:], CNT0 + cut)
        assert bytes(st) == want, cut
    st = gc.G1FrameState(ephcnt=2)
    for r in range(len(log)):
        gc.g1frame_replay(st, log[r:r + 1], CNT0 + r)
    assert bytes(st) == want


# ---- time ------------------------------------------------------------------------------------------------------------
def _lib_time(gc, nt, n4, tk):
    """(week, tow_gpst - 10) of strings 1..5 through the library."""
    sym, _ = gs.stream([1, 2, 3, 4, 5], 50, tk=tk, nt=nt, n4=n4)
    st = gc.G1FrameState()
    gc.g1frame_replay(st, gs.log_rows(gc, sym), 0)
    assert (st.flagdec, st.s1cnt, st.nt, st.n4) == (1, 5, nt, n4)
    assert list(st.tk) == [tk[0] - 3, tk[1], 30 * tk[2]]
    return st.week, st.tow_gpst - 10.0


def test_time_equals_datetime_arithmetic(gc):
    """Second to fourth year of an interval, January to November, 2010-2024: first, 15th and last day of each month, at
    Moscow times on both sides of the UTC date line."""
    import calendar
    n = 0
    for year in range(2010, 2025):
        if year % 4 == 0:
            continue
        for month in range(1, 12):
            for day in (1, 15, calendar.monthrange(year, month)[1]):
                tk = [(1, 59, 1), (14, 25, 0), (23, 0, 1)][n % 3]
                nt, n4 = gs.glonass_day(year, month, day)
                want = gs.gps_week_tow(year, month, day, tk[0], tk[1], 30 * tk[2])
                week, tow = gr.time2gpst(gr.glot2time(nt, n4, [tk[0] - 3, tk[1], 30 * tk[2]]))
                assert (week, tow) == want, (year, month, day)
                if n % 7 == 0:
                    assert _lib_time(gc, nt, n4, tk) == (want[0], float(want[1])), (year, month, day)
                n += 1
    assert n == 11 * 11 * 3


def test_time_quirks(gc):
    """What glot2time() does outside that range, pinned: in the first (leap) year of an interval the date is the day
    before; every December date is the 30th of November; a day number past 1461 is the year before the interval."""
    for (y, mo, d) in [(2020, 1, 1), (2020, 2, 29), (2020, 3, 1), (2024, 7, 10), (2016, 11, 30)]:
        nt, n4 = gs.glonass_day(y, mo, d)
        assert nt <= 366
        week, tow = gs.gps_week_tow(y, mo, d, 14, 25, 30)
        w, t = (week, tow - 86400) if tow >= 86400 else (week - 1, tow + 6 * 86400)
        assert _lib_time(gc, nt, n4, (14, 25, 1)) == (w, float(t)) == gr.time2gpst(gr.glot2time(nt, n4, [11, 25, 30]))
    for (y, mo, d) in [(2021, 12, 1), (2023, 12, 31), (2020, 12, 1), (2020, 12, 31)]:
        nt, n4 = gs.glonass_day(y, mo, d)
        assert gr.glo_date(nt, n4) == (y, 12, 0)
        week, tow = gs.gps_week_tow(y, 11, 30, 14, 25, 30)
        assert _lib_time(gc, nt, n4, (14, 25, 1)) == (week, float(tow))
    assert gr.glo_date(1462, 7) == (2019, 1, -1) and gr.glo_date(0, 7) == (2020, 1, -1)
    for nt, n4 in [(1462, 7), (2047, 7), (0, 7), (100, 0), (100, 31)]:           # (n4 = 31: past 2099, epoch2time gives 0)
        week, tow = gr.time2gpst(gr.glot2time(nt, n4, [11, 25, 30]))
        assert _lib_time(gc, nt, n4, (14, 25, 1)) == (week, float(tow))
    assert gr.time2gpst(gr.glot2time(100, 31, [11, 25, 30])) == (-522, -259200)


# ---- memory safety: the stand-alone program under sanitizers ---------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("g1host") / "g1frame_host")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",     # (no runtime to load first)
                           os.path.join(ROOT, "tests", "host", "g1frame_host.c"),
                           os.path.join(ROOT, "erlangnetwork-gnsslib-sdr_amd", "csrc", "sdr_g1.c"), "-o", exe])
    return exe


def _parse(line):
    t = line.split()
    ints = [int(v) for v in t[:19]]
    names = ("row", "polarity", "flagsyncf", "flagtow", "flagdec", "id", "ephcnt", "s1cnt", "tk0", "tk1", "tk2", "nt", "slot",
             "n4", "iode", "update", "week", "firstsf", "firstsfcnt")
    d = dict(zip(names, ints))
    d["tk"] = [d.pop("tk0"), d.pop("tk1"), d.pop("tk2")]
    d.update(firstsftow=float(t[19]), tow_gpst=float(t[20]), str=bytes.fromhex(t[21]), fbits=[{"+": 1, "-": -1, "0": 0}[c] for c in t[22]])
    return d


@pytest.mark.parametrize("name, piece, zero_at", [("frame", 777, -1), ("frame", 14000, -1), ("noise", 1, -1), ("twice", 10000, 10000)])
def test_standalone_program_under_sanitizers(host_exe, tmp_path, name, piece, zero_at):
    if name == "noise":                         # any symbols, zeros among them, row by row
        rows = np.random.default_rng(3).integers(-1, 2, size=3000).astype(np.int8)
        rows[1000:1030] = gr.MARK
    else:
        numbers = [6, 7, 3, 4, 5, 1, 2] if name == "frame" else [1, 2, 3, 4, 5] * 2
        sym, _ = gs.stream(numbers, 60, polarity=-1, **FIELDS)
        rows = np.zeros(10 * len(sym), np.int8)
        rows[FIRST::10] = sym
    path = tmp_path / "rows.bin"
    rows.tofile(path)
    args = [host_exe, str(path), str(CNT0), str(piece)] + ([str(zero_at)] if zero_at >= 0 else [])
    out = subprocess.run(args, capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == -(-len(rows) // piece)
    rep = gr.G1Replay()
    loc = 1000 * (CNT0 + np.arange(len(rows)))
    for k, line in enumerate(lines):
        a = k * piece
        if a == zero_at:
            rep.ephcnt = 0
        rep.run_log(rows[a:a + piece], loc[a:a + piece], CNT0 + a)
        got = _parse(line)
        assert got.pop("row") == min(a + piece, len(rows)) and got == rep.fields(), k
    if name == "frame":
        assert (rep.flagdec, rep.firstsftow, rep.polarity) == (1, TOW1 + 4.0, -1)
    if name == "twice":
        assert (rep.ephcnt, rep.s1cnt, rep.tow_gpst) == (5, 5, TOW1 + 10.0)
