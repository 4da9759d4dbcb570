"""gnsscorr_rxnav_* on the CPU (no GPU): the driver of csrc/sdr_rxnav.c against the reference composition
tests/rxnav_cases.py::Compose -- the feed's six rules written out from gc.frame_replay,
gc.g1frame_replay, gc.obs_replay and gc.Sync -- over the same arrays: status, frame states byte for byte, the rows of
every feed and the epochs, all as equalities.  The inputs are the oracle's logs of tests/sync_if_cases.py (three L1 C/A
satellites) and tests/g1_if_cases.py (GLONASS G1), and small hand-made logs for the rules.  Memory safety: the
stand-alone program tests/host/rxnav_host.c, plain and under address and undefined-behaviour sanitizers, run as a child
process; nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import g1_if_cases as gic
import g1_restate as gr
import rxnav_cases as rc
import sync_if_cases as sic
import sync_restate as sr
from test_sync_if_host import BAR_M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 40


def both(gc, chans, outms, hold):
    return gc.RxNav(chans, outms, hold), rc.Compose(gc, chans, outms, hold)


def feed_both(gc, nav, cmp, logs, stride, cnt_after, tracking, where=""):
    log, ii, ndone = rc.pack(gc, logs, stride)
    nav.feed(log, ii, ndone, cnt_after, tracking)
    cmp.feed(log, ii, ndone, cnt_after, tracking)
    rc.assert_same(gc, nav, cmp, where)
    return rc.assert_same_epochs(nav, cmp, where)


# ---- three L1 C/A satellites ---------------------------------------------------------------------------------------------
def l1ca_feeds(gc, orc, synth):
    """[(logs per channel, cnt_after)] of the oracle's run cut in sic.PIECES."""
    runs, a, out = sic.oracle_run(gc, orc, synth), 0, []
    for n in sic.PIECES:
        out.append(([(log[a:a + n], I[a:a + n]) for log, I in runs], [sic.CNT0[i] + a + n for i in range(3)]))
        a += n
    return out


def test_three_l1ca_satellites_equal_compose_and_give_the_known_epochs(gc, orc, synth):
    chans = [rc.chan_of(gc, ch) for ch in sic.channels(gc)]
    nav, cmp = both(gc, chans, sic.OUTMS, 0)
    for k in range(3):
        nav.week(k, sic.WEEK)
        cmp.week(k, sic.WEEK)
    out = []
    for n, (logs, cnt_after) in enumerate(l1ca_feeds(gc, orc, synth)):
        out += feed_both(gc, nav, cmp, logs, len(logs[0][0]), cnt_after, [1, 1, 1], "piece %d" % n)
    nav.flush()
    cmp.flush()
    out += rc.assert_same_epochs(nav, cmp, "flush")
    st = nav.status(3)
    for i in range(3):
        assert (st["flagdec"][i], st["id"][i], st["firstsftow"][i], st["week"][i]) == (1, sic.SFID, sic.FIRSTSFTOW, sic.WEEK)
        assert st["firstsfcnt"][i] == sic.CNT0[i] + sic.found_row(i) and st["attached"][i] == 1 and st["resets"][i] == 0
    # compose is the caller's loop the existing tests write out: the rows and frame fields of sic.replays, push for push
    per = [sic.replays(gc, i, sic.cut(log), I)[1] for i, (log, I) in enumerate(sic.oracle_run(gc, orc, synth))]
    assert [(p[0]) for p in cmp.pushes] == [0, 1, 2] * 3
    for n in range(3):
        for i in range(3):
            _, sf, rows = cmp.pushes[3 * n + i]
            want_sf, want_rows = per[i][n]
            assert rc.same_rows(rows, want_rows), (n, i)
            assert (sf.flagdec, sf.firstsf, sf.firstsfcnt) == (want_sf.flagdec, want_sf.firstsf, want_sf.firstsfcnt)
    # the epochs tests/test_sync_if_host.py knows; that the channels attach one after the other changes none of them
    assert sr.same_bits(out, sic.restated(cmp.pushes))
    eps = sic.full_epochs(out)
    assert [k for k, _ in eps] == list(range(1, sic.NROWS_AFTER + 1))
    worst = sic.worst_range_error(eps)
    print("driver over the oracle's logs: %d epochs, worst |P_i - P_j - truth| = %.3f m (bar %.1f m)" % (len(eps), worst, BAR_M))
    assert worst < BAR_M
    nav.close()
    cmp.close()


# ---- GLONASS G1 with an absent channel -------------------------------------------------------------------------------
def g1_log(gc, r):
    """The oracle's log as tests/test_g1_if_host.py builds it (navbit, buffloc, flagsync), with the columns the
    observables read filled in: a prm2 filter update in every row that decides a symbol (every loopms = 10 periods from
    bit synchronisation on), the carrier frequency the oracle ended on, the nominal code rate and period length."""
    log = np.zeros(gic.NPER, dtype=np.dtype(gc.TrkLog))
    log["navbit"], log["buffloc"], log["flagsync"] = r["navbit"], r["buffloc"], r["flagsync"]
    log["flagloopfilter"] = np.where(r["navbit"] != 0, 2, 0)
    log["carrfreq"], log["codefreq"], log["currnsamp"] = r["carrfreq"], 0.511e6, gic.NSAMP
    return log


def g1_feeds(gc, orc, synth, name="phase0.7"):
    r, c = gic.oracle_run(gc, orc, synth, name), gic.case(name)
    log, a, out = g1_log(gc, r), 0, []
    for n in gic.CHUNKS:
        out.append(([(log[a:a + n], r["I"][a:a + n]), None], [c["cnt0"] + a + n, 0]))
        a += n
    return out, r, c


def test_g1_with_an_absent_channel(gc, orc, synth):
    chans = [rc.chan_of(gc, gic.channel(gc)), rc.chan_of(gc, gic.channel(gc, freqno=2))]
    nav, cmp = both(gc, chans, 10, 2)
    feeds, r, c = g1_feeds(gc, orc, synth)
    out = []
    for n, (logs, cnt_after) in enumerate(feeds):
        out += feed_both(gc, nav, cmp, logs, len(logs[0][0]), cnt_after, [1, 1], "chunk %d" % n)
    nav.flush()
    cmp.flush()
    out += rc.assert_same_epochs(nav, cmp, "flush")
    st = nav.frame(0, gc.CTYPE_G1)
    assert gr.state_fields(st) == gic.replayed(r["navbit"], r["buffloc"]).fields()
    assert (st.flagdec, st.week, st.firstsftow, st.firstsfcnt) == (1, gic.WEEK, gic.FIRSTSFTOW, c["cnt0"] + gic.FOUND_ROW)
    assert len(out) >= 1 and all((e[0], e[1]) == (0, gic.WEEK) for e in out)
    assert out[0][2] == gic.FIRSTSFTOW + sr.PTIMING / 1000
    s = nav.status(2)
    assert (s["attached"][0], s["week"][0], s["nrows"][0]) == (1, gic.WEEK, int(np.count_nonzero(r["navbit"])))
    assert (s["attached"][1], s["resets"][1], s["nrows"][1], s["cnt"][1], s["flagdec"][1]) == (0, 0, 0, 0, 0)
    assert bytes(nav.frame(1, gc.CTYPE_G1)) == bytes(C.sizeof(gc.G1FrameState))
    nav.close()
    cmp.close()


# ---- the rules, on small hand-made logs ------------------------------------------------------------------------------
def two(gc):
    return [rc.chan_of(gc, ch) for ch in sic.channels(gc)[:2]]


def snapshot(gc, nav, nch=2):
    return rc.status_of(nav, nch), [bytes(nav.frame(k, gc.CTYPE_L1CA)) for k in range(nch)], [nav.rows(k).tobytes() for k in range(nch)]


def test_a_gap_in_cnt_is_refused_and_touches_nothing(gc):
    nav, cmp = both(gc, two(gc), 10, 0)
    a, b = rc.hand_log(gc, STRIDE, 0), rc.hand_log(gc, STRIDE, 500, buffloc0=1777)
    feed_both(gc, nav, cmp, [a, b], STRIDE, [40, 540], [1, 1])
    before = snapshot(gc, nav)
    log, ii, ndone = rc.pack(gc, [rc.hand_log(gc, STRIDE, 40), rc.hand_log(gc, STRIDE, 580, buffloc0=1777)], STRIDE)
    with pytest.raises(gc.GnsscorrError) as e:
        nav.feed(log, ii, ndone, [80, 620], [1, 1])             # channel 1: rows 580.. behind a feed that ended at 540
    assert e.value.code == gc.ESTATE and "channel 1" in str(e.value)
    with pytest.raises(rc.SkippedRows):
        cmp.feed(log, ii, ndone, [80, 620], [1, 1])
    assert snapshot(gc, nav) == before
    rc.assert_same(gc, nav, cmp)
    # the rows that do continue are taken
    feed_both(gc, nav, cmp, [rc.hand_log(gc, STRIDE, 40), rc.hand_log(gc, STRIDE, 540, buffloc0=1777)], STRIDE, [80, 580], [1, 1])
    assert list(nav.status(2)["nrows"]) == [8, 8]
    nav.close()
    cmp.close()


def test_tracking_0_zeroes_detaches_and_counts_one_reset(gc):
    nav, cmp = both(gc, two(gc), 10, 0)
    feed_both(gc, nav, cmp, [rc.hand_log(gc, STRIDE, 0), rc.hand_log(gc, STRIDE, 0, buffloc0=1777)], STRIDE, [40, 40], [1, 1])
    assert list(nav.status(2)["attached"]) == [1, 1] and list(nav.status(2)["nrows"]) == [4, 4]
    feed_both(gc, nav, cmp, [rc.hand_log(gc, STRIDE, 40), None], STRIDE, [80, 40], [1, 0])
    st = nav.status(2)
    assert (st["attached"][1], st["resets"][1], st["nrows"][1], st["tow"][1]) == (0, 1, 0, 0.0) and st["nrows"][0] == 8
    # an empty state is zeroed again without counting
    feed_both(gc, nav, cmp, [rc.hand_log(gc, STRIDE, 80), None], STRIDE, [120, 40], [1, 0])
    assert nav.status(2)["resets"][1] == 1
    # rows of a channel that is not tracking are dropped
    feed_both(gc, nav, cmp, [rc.hand_log(gc, STRIDE, 120), rc.hand_log(gc, STRIDE, 0, buffloc0=999777)], STRIDE, [160, 40], [1, 0])
    assert (nav.status(2)["nrows"][1], nav.status(2)["attached"][1], nav.status(2)["resets"][1]) == (0, 0, 1)
    nav.close()
    cmp.close()


def test_cnt0_zero_after_rows_zeroes(gc):
    nav, cmp = both(gc, two(gc), 10, 0)
    feed_both(gc, nav, cmp, [rc.hand_log(gc, STRIDE, 0), rc.hand_log(gc, STRIDE, 7, buffloc0=1777)], STRIDE, [40, 47], [1, 1])
    feed_both(gc, nav, cmp, [rc.hand_log(gc, STRIDE, 40), rc.hand_log(gc, 25, 0, buffloc0=9001777)], STRIDE, [80, 25], [1, 1])
    st = nav.status(2)
    assert (st["resets"][0], st["nrows"][0]) == (0, 8) and (st["resets"][1], st["nrows"][1], st["attached"][1]) == (1, 2, 1)
    nav.close()
    cmp.close()


@pytest.mark.parametrize("hold", [0, 1, 2])
def test_starved_channels_are_detached_after_hold_steps(gc, hold):
    nav, cmp = both(gc, two(gc), 10, hold)
    feed_both(gc, nav, cmp, [rc.hand_log(gc, STRIDE, 0), rc.hand_log(gc, STRIDE, 0, buffloc0=1777)], STRIDE, [40, 40], [1, 1])
    # feeds without rows for anyone starve no one
    for _ in range(3):
        feed_both(gc, nav, cmp, [None, None], STRIDE, [40, 40], [1, 1])
        assert list(nav.status(2)["attached"]) == [1, 1]
    seen = []
    for n in range(1, 4):
        feed_both(gc, nav, cmp, [rc.hand_log(gc, STRIDE, 40 * n), None], STRIDE, [40 * n + 40, 40], [1, 1])
        seen.append(int(nav.status(2)["attached"][1]))
    assert seen == {0: [1, 1, 1], 1: [0, 0, 0], 2: [1, 0, 0]}[hold]
    st = nav.status(2)
    assert (st["nrows"][1], st["resets"][1], st["attached"][0]) == (4, 0, 1)        # its nav state stays
    # a feed in which nobody had rows between two starved ones starts the count again
    if hold == 2:
        feed_both(gc, nav, cmp, [rc.hand_log(gc, STRIDE, 160), rc.hand_log(gc, STRIDE, 40, buffloc0=1777)], STRIDE, [200, 80], [1, 1])
        for logs, cnt in [([rc.hand_log(gc, STRIDE, 200), None], 240), ([None, None], 240), ([rc.hand_log(gc, STRIDE, 240), None], 280)]:
            feed_both(gc, nav, cmp, logs, STRIDE, [cnt, 80], [1, 1])
        assert nav.status(2)["attached"][1] == 1
    nav.close()
    cmp.close()


def test_refusals(gc):
    L = gc.lib()
    chans = two(gc)
    # an SBAS channel without a context
    nav = gc.RxNav([chans[0], dict(chans[1], ctype=gc.CTYPE_L1SBAS)], 10, 0)
    log, ii, ndone = rc.pack(gc, [rc.hand_log(gc, STRIDE, 0), None], STRIDE)
    before = rc.status_of(nav, 2)
    with pytest.raises(gc.GnsscorrError) as e:
        nav.feed(log, ii, ndone, [40, 0], [1, 1])
    assert e.value.code == gc.EINVAL and "channel 1" in str(e.value) and rc.status_of(nav, 2) == before
    nav.close()
    # a ti mismatch fails in create with the sync's message
    s = gc.Sync(2, 10)
    s.channel(0, chans[0]["nsamp"], chans[0]["ctime"], chans[0]["ti"])
    with pytest.raises(gc.GnsscorrError) as se:
        s.channel(1, chans[1]["nsamp"], chans[1]["ctime"], 1 / 4.0e6)
    s.close()
    with pytest.raises(gc.GnsscorrError) as e:
        gc.RxNav([chans[0], dict(chans[1], ti=1 / 4.0e6)], 10, 0)
    assert e.value.code == se.value.code == gc.EINVAL and str(se.value) and str(se.value) in str(e.value)
    # a code type outside the three; bad counts
    for bad in (dict(chans[1], ctype=0), dict(chans[1], ctype=2)):
        with pytest.raises(gc.GnsscorrError) as e:
            gc.RxNav([chans[0], bad], 10, 0)
        assert e.value.code == gc.EINVAL and "channel 1" in str(e.value)
    nav = gc.RxNav(chans, 10, 0)
    cnt, trk = np.array([40, 0], np.uint64), np.array([1, 1], np.int32)
    for ndone_bad, stride in [([40, -1], STRIDE), ([40, 0], STRIDE - 1)]:
        nd = np.array(ndone_bad, np.int32)
        assert L.gnsscorr_rxnav_feed(nav.h, None, log.ctypes.data, ii.ctypes.data, stride, nd.ctypes.data, cnt.ctypes.data,
                                     trk.ctypes.data) == gc.EINVAL
    # a wrong size in gnsscorr_rxnav_frame
    fr = gc.FrameState()
    assert L.gnsscorr_rxnav_frame(nav.h, 0, C.byref(fr), C.sizeof(fr) - 4) == gc.EINVAL
    assert L.gnsscorr_rxnav_frame(nav.h, 0, C.byref(gc.G1FrameState()), C.sizeof(gc.G1FrameState)) == gc.EINVAL
    assert L.gnsscorr_rxnav_frame(nav.h, 0, C.byref(fr), C.sizeof(fr)) == 0
    with pytest.raises(gc.GnsscorrError):
        nav.week(2, 1)
    nav.close()


def test_layout(gc):
    assert C.sizeof(gc.RxNavCh) == 64 and C.sizeof(gc.RxNavStat) == 80 and gc.RxNavStat.cnt.offset == 32
    hdr = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    assert "first row of the piece that raised flagdec" in hdr          # the one dependence on the cut is stated there


# ---- the stand-alone program -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rxnavhost") / ("rxnav_host_" + request.param))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                      "-static-libasan", "-static-libubsan"]      # (no runtime to load first)
    csrc = os.path.join(ROOT, "erlangnetwork-gnsslib-sdr_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-ffp-contract=off"] + flags +
                          [os.path.join(ROOT, "tests", "host", "rxnav_host.c")] +
                          [os.path.join(csrc, f) for f in ("sdr_rxnav.c", "sdr_host.c", "sdr_g1.c", "sdr_sync.c")] +
                          ["-o", exe, "-lm", "-lpthread"])
    return exe


def script_create(chans, outms, hold):
    lines = ["create %d %d %d" % (len(chans), outms, hold)]
    for c in chans:
        lines.append("%d %d %d " % (c["ctype"], c["nsamp"], c["loopms"]) +
                     " ".join(float(c[n]).hex() for n in ("f_sf", "f_if", "foffset", "ctime", "ti", "oldremcode")))
    return lines


def script_feed(logs, stride, cnt_after, tracking):
    lines = ["feed %d" % stride]
    for k, l in enumerate(logs):
        n = 0 if l is None else len(l[0])
        lines.append("%d %d %d" % (n, cnt_after[k], tracking[k]))
        for p in range(n):
            r = l[0][p]
            lines.append(" ".join(float(r[f]).hex() for f in ("carrfreq", "codefreq", "remcode", "remcarr")) +
                         " %d %d %d %d %d " % (r["buffloc"], r["currnsamp"], r["flagloopfilter"], r["flagsync"], r["navbit"]) +
                         float(l[1][p]).hex())
    return lines


def run_script(exe, tmp_path, lines):
    path = tmp_path / "script.txt"
    path.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stderr[-2000:])
    out = dict(rc=[], row=[], epo=[], st=[], fr=[])
    for line in res.stdout.splitlines():
        t = line.split()
        if t[0] == "rc":
            out["rc"].append(int(t[1]))
        elif t[0] == "row":
            out["row"].append((int(t[1]),) + tuple(float.fromhex(v) for v in t[2:7]) + tuple(int(v) for v in t[7:10]))
        elif t[0] == "epo":
            out["epo"].append((int(t[1]), int(t[2])) + tuple(float.fromhex(v) for v in t[3:8]) + (int(t[8]),))
        elif t[0] == "st":
            out["st"].append(tuple(int(v) for v in t[1:13]) + tuple(float.fromhex(v) for v in t[13:15]))
        elif t[0] == "fr":
            out["fr"].append((int(t[1]), t[2]))
    return out


def library_run(gc, chans, outms, hold, weeks, feeds, tracking):
    """The same calls through the library loaded here: what the program must print."""
    nav = gc.RxNav(chans, outms, hold)
    for k, w in weeks:
        nav.week(k, w)
    rows = []
    for logs, cnt_after in feeds:
        log, ii, ndone = rc.pack(gc, logs, max(len(l[0]) for l in logs if l is not None))
        nav.feed(log, ii, ndone, cnt_after, tracking)
        for k in range(len(chans)):
            rows += [(k,) + tuple(float(r[n]) for n in ("tow", "remcout", "L", "D", "S")) + (int(r["codei"]), int(r["cntout"]), int(r["snr"]))
                     for r in nav.rows(k)]
    nav.flush()
    want = dict(row=rows, epo=sr.out_of(nav.fetch()), st=rc.status_of(nav, len(chans)),
                fr=[(k, bytes(nav.frame(k, c["ctype"])).hex()) for k, c in enumerate(chans)])
    nav.close()
    return want


@pytest.mark.parametrize("which", ["l1ca", "g1"])
def test_standalone_program(gc, orc, synth, host_exe, tmp_path, which):
    """csrc/sdr_rxnav.c with the host files it needs and stubs for the device (once plain, once under the sanitizers):
    its built-in error paths, then a whole log through create / week / feed / fetch / status / frame / destroy, equal
    to the library's answers."""
    if which == "l1ca":
        chans, outms, hold, tracking = [rc.chan_of(gc, ch) for ch in sic.channels(gc)], sic.OUTMS, 0, [1, 1, 1]
        weeks, feeds = [(k, sic.WEEK) for k in range(3)], l1ca_feeds(gc, orc, synth)
    else:
        chans, outms, hold, tracking = [rc.chan_of(gc, gic.channel(gc)), rc.chan_of(gc, gic.channel(gc, freqno=2))], 10, 2, [1, 1]
        weeks, feeds = [], g1_feeds(gc, orc, synth)[0]
    lines = script_create(chans, outms, hold) + ["week %d %d" % kw for kw in weeks]
    for logs, cnt_after in feeds:
        lines += script_feed(logs, max(len(l[0]) for l in logs if l is not None), cnt_after, tracking)
    lines += ["flush", "fetch", "status"] + ["frame %d" % k for k in range(len(chans))] + ["destroy"]
    got = run_script(host_exe, tmp_path, lines)
    want = library_run(gc, chans, outms, hold, weeks, feeds, tracking)
    assert got["rc"] == [0] * (1 + len(weeks) + len(feeds) + 3 + len(chans) + 1)
    assert len(want["row"]) > 100 and len(want["epo"]) >= 1
    assert sr.same_bits(got["row"], want["row"]) and sr.same_bits(got["epo"], want["epo"]) and sr.same_bits(got["st"], want["st"])
    assert got["fr"] == want["fr"]
