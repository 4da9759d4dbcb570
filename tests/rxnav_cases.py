"""Helpers of tests/test_rxnav_host.py and tests/test_gpu_rx_nav.py (not a conftest): the reference composition of
gnsscorr_rxnav_feed -- the feed's six rules written out in Python from the public calls
gc.frame_replay, gc.g1frame_replay, Engine.sbasframe_replay, gc.obs_replay and gc.Sync -- and what compares a driver
with it."""
import ctypes as C

import numpy as np

import sync_restate as sr

STAT_FIELDS = ("ctype", "attached", "flagsyncf", "flagdec", "polarity", "week", "id", "resets", "cnt", "firstsf",
               "firstsfcnt", "nrows", "firstsftow", "tow")


class SkippedRows(Exception):
    """compose's GNSSCORR_ESTATE: a channel's rows do not continue the feed before."""


def chan_of(gc, ch, loopms=10, oldremcode=0.0):
    """The RxNavCh fields of a gc.Channel."""
    return dict(ctype=ch.ctype, nsamp=ch.nsamp, loopms=loopms, f_sf=ch.f_sf, f_if=ch.f_if, foffset=ch.foffset, ctime=ch.ctime,
                ti=ch.ti, oldremcode=oldremcode)


class Compose:
    """compose(...): one object per receiver, feed() per step.  `chans`: dicts of the RxNavCh fields."""

    def __init__(self, gc, chans, outms, hold_steps):
        self.gc, self.cfg, self.hold = gc, [dict(c) for c in chans], hold_steps
        self.sync = gc.Sync(len(chans), outms)
        self.ch, self.pushes = [], []           # pushes: every (ch, SyncFrame, rows) pushed, in order
        for k, c in enumerate(self.cfg):
            self.sync.channel(k, c["nsamp"], c["ctime"], c["ti"])
            self.sync.detach(k)                 # declared, and detached until it delivers
            self.ch.append(dict(fr=self._frame(c), ob=self._obs(c, c.get("oldremcode", 0.0)), attached=0, resets=0, week=0, fed=False,
                                held=False, starved=0, cnt=0, nrows=0, tow=0.0, rows=np.zeros(0, np.dtype(gc.ObsRow))))

    def close(self):
        self.sync.close()

    def _frame(self, c):
        gc = self.gc
        return {gc.CTYPE_L1CA: gc.FrameState, gc.CTYPE_G1: gc.G1FrameState, gc.CTYPE_L1SBAS: gc.SbasFrameState}[c["ctype"]]()

    def _obs(self, c, oldremcode):
        st = self.gc.ObsState()
        st.f_sf, st.f_if, st.foffset, st.ctime, st.loopms, st.oldremcode = c["f_sf"], c["f_if"], c["foffset"], c["ctime"], c["loopms"], oldremcode
        return st

    def week(self, k, week):
        self.ch[k]["week"] = week

    def _reset(self, k):
        s, c = self.ch[k], self.cfg[k]
        s["resets"] += int(s["held"])
        s.update(fr=self._frame(c), ob=self._obs(c, 0.0), nrows=0, tow=0.0, starved=0, held=False, attached=0)
        self.sync.detach(k)

    def _week_of(self, k):
        return self.ch[k]["week"] if self.cfg[k]["ctype"] == self.gc.CTYPE_L1CA else int(self.ch[k]["fr"].week)

    def feed(self, log, II0, ndone, cnt_after, tracking, eng=None):
        gc = self.gc
        nch = len(self.ch)
        for k in range(nch):
            cnt0 = int(cnt_after[k]) - int(ndone[k])
            if ndone[k] > 0 and self.ch[k]["fed"] and cnt0 != 0 and cnt0 != self.ch[k]["cnt"]:
                raise SkippedRows(k)
        some = sum(int(n > 0) for n in ndone)
        for k in range(nch):
            s, c, n = self.ch[k], self.cfg[k], int(ndone[k])
            cnt0 = int(cnt_after[k]) - n
            # 1. reset
            if not tracking[k] or (n > 0 and cnt0 == 0 and s["held"]):
                self._reset(k)
            s["fed"], s["cnt"], s["rows"] = True, int(cnt_after[k]), np.zeros(0, np.dtype(gc.ObsRow))
            if n > 0 and tracking[k]:
                rows, fr = np.ascontiguousarray(log[k][:n]), s["fr"]
                # 2. the frame replay of the code type
                if c["ctype"] == gc.CTYPE_L1CA:
                    gc.frame_replay(fr, rows, cnt0=cnt0)
                elif c["ctype"] == gc.CTYPE_G1:
                    gc.g1frame_replay(fr, rows, cnt0=cnt0)
                else:
                    eng.sbasframe_replay(fr, rows, cnt0=cnt0)
                s["held"] = True
                # 3. the frame fields, before the piece that raised flagdec
                ob = s["ob"]
                if fr.flagdec:
                    ob.flagsyncf, ob.polarity, ob.firstsftow, ob.firstsfcnt = fr.flagsyncf, fr.polarity, fr.firstsftow, fr.firstsfcnt
                # 4. observables
                obs = gc.obs_replay(ob, rows, np.ascontiguousarray(II0[k][:n]), cnt0=cnt0)
                s["rows"] = obs.copy()
                s["nrows"] += len(obs)
                # 5. push
                if len(obs):
                    s["tow"] = float(obs["tow"][-1])
                    sf = gc.SyncFrame(int(fr.flagdec), self._week_of(k), int(fr.firstsf), int(fr.firstsfcnt))
                    self.sync.push(k, sf, obs)
                    self.pushes.append((k, sf, obs.copy()))
                    s["attached"] = 1
            # 6. starvation
            if n == 0 and tracking[k] and s["attached"] and some > 0:
                s["starved"] += 1
                if self.hold > 0 and s["starved"] >= self.hold:
                    self.sync.detach(k)
                    s["attached"], s["starved"] = 0, 0
            else:
                s["starved"] = 0

    def flush(self):
        self.sync.flush()

    def fetch(self):
        return self.sync.fetch()

    def status(self):
        """Per channel the tuple in the order of STAT_FIELDS."""
        gc, out = self.gc, []
        for k, (s, c) in enumerate(zip(self.ch, self.cfg)):
            fr = s["fr"]
            ident = fr.sfid if c["ctype"] == gc.CTYPE_L1CA else fr.id
            out.append((c["ctype"], s["attached"], fr.flagsyncf, fr.flagdec, fr.polarity, self._week_of(k), ident, s["resets"], s["cnt"],
                        fr.firstsf, fr.firstsfcnt, s["nrows"], fr.firstsftow, s["tow"]))
        return out


def status_of(nav, nch):
    """The driver's status as compose's tuples."""
    st = nav.status(nch)
    return [tuple(st[n][k].item() for n in STAT_FIELDS) for k in range(nch)]


def same_rows(a, b):
    """Two arrays of ObsRow, bit for bit."""
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same(gc, nav, cmp, where=""):
    """The driver's state against compose's: status, frame states byte for byte, the rows of the last feed."""
    nch = len(cmp.ch)
    got, want = status_of(nav, nch), cmp.status()
    for k in range(nch):
        assert sr.same_bits([got[k]], [want[k]]), (where, k, got[k], want[k])
        assert bytes(nav.frame(k, cmp.cfg[k]["ctype"])) == bytes(cmp.ch[k]["fr"]), (where, k)
        assert same_rows(nav.rows(k), cmp.ch[k]["rows"]), (where, k)


def assert_same_epochs(nav, cmp, where=""):
    """The epochs both have made since the last look; returns them as sync_restate's tuples."""
    got, want = sr.out_of(nav.fetch()), sr.out_of(cmp.fetch())
    assert sr.same_bits(got, want), (where, len(got), len(want))
    return got


def hand_log(gc, nper, cnt0, buffloc0=1000, nsamp=4092, loopms=10, carrfreq=1000.0, codefreq=1.023e6):
    """A small hand-made log of one channel: bit columns zero, a prm2 filter update (a row of observables) wherever
    cnt % loopms == loopms - 1, a prm1 update elsewhere; and its II0."""
    log = np.zeros(nper, dtype=np.dtype(gc.TrkLog))
    cnt = cnt0 + np.arange(nper)
    log["buffloc"] = buffloc0 + nsamp * cnt
    log["currnsamp"], log["carrfreq"], log["codefreq"], log["flagsync"] = nsamp, carrfreq, codefreq, 1
    log["remcode"] = 0.125 + (cnt % 7) / 64.0
    log["remcarr"] = 0.5
    log["flagloopfilter"] = np.where(cnt % loopms == loopms - 1, 2, 0)
    return log, 1000.0 + (cnt % 3).astype(np.float64)


def pack(gc, logs, stride):
    """[(log, II0) or None per channel] -> log [nch][stride], II0 [nch][stride], ndone [nch]."""
    log, ii, ndone = np.zeros((len(logs), stride), np.dtype(gc.TrkLog)), np.zeros((len(logs), stride)), np.zeros(len(logs), np.int32)
    for k, l in enumerate(logs):
        if l is not None:
            n = len(l[0])
            log[k, :n], ii[k, :n], ndone[k] = l[0], l[1], n
    return log, ii, ndone
