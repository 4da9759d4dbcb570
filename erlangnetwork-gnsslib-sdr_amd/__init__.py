"""Host-side Python mirror of libgnsscorr.so (MI355X GNSS correlation engine).

The product is the C-ABI shared library built from ``csrc/`` (HIP kernels for
gfx950 + C host code); this package only binds it with ctypes so that tests,
``bench.py`` and ``__graft_entry__.py`` can drive it, and mirrors the
reference's channel set-up (``initsdrch``, ref src/sdrinit.c:583-657) so that
call sites read like the reference's.  There is no CPU fallback: importing
works without a GPU, but every compute entry point fails loudly when the
library or a device is missing.

The directory name contains '-', so it is loaded through ``gnsscorr_loader``
(repo root) under the module name ``erlangnetwork_gnsslib_sdr_amd``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GNSSCORR_LIB", os.path.join(_HERE, "libgnsscorr.so"))   # override: A/B builds

MAXTAPS = 33
FMT_STEREO, FMT_RTLSDR = 1, 2
CTYPE_L1CA, CTYPE_G1, CTYPE_L1SBAS = 1, 20, 27
SYS_GPS, SYS_SBS, SYS_GLO = 1, 2, 4
DTYPEI, DTYPEIQ = 1, 2
FTYPE1, FTYPE2 = 1, 2
FEND_RTLSDR, FEND_FRTLSDR, FEND_FILE = 3, 8, 10
MEMBUFFLEN, FILE_BUFFSIZE = 5000, 65536      # ref src/sdr.h:134,137
ACQTH = 3.0                                  # ref src/sdr.h:148
MAXFREQ, MAXCOH = 1024, 20                   # GNSSCORR_MAXFREQ, GNSSCORR_MAXCOH
FINE_BINS = 256                              # GNSSCORR_FINE_BINS


class GnsscorrError(RuntimeError):
    pass


# ---- ctypes mirrors of include/gnsscorr.h ---------------------------------
class ChanDesc(C.Structure):
    _fields_ = [("prn", C.c_int), ("ctype", C.c_int), ("dtype", C.c_int), ("ftype", C.c_int),
                ("clen", C.c_int), ("nsamp", C.c_int), ("nsampchip", C.c_int),
                ("f_sf", C.c_double), ("f_if", C.c_double), ("foffset", C.c_double),
                ("crate", C.c_double), ("ctime", C.c_double), ("ti", C.c_double),
                ("code", C.POINTER(C.c_short)), ("intg", C.c_int), ("nfreq", C.c_int),
                ("freq", C.POINTER(C.c_double)), ("nfft", C.c_int), ("corrn", C.c_int),
                ("corrp", C.POINTER(C.c_int))]


class TrkState(C.Structure):
    _fields_ = [("carrfreq", C.c_double), ("codefreq", C.c_double), ("remcode", C.c_double),
                ("remcarr", C.c_double), ("buffloc", C.c_uint64)]




class LoopState(C.Structure):
    """gnsscorr_loop_t (include/gnsscorr.h): loop-filter configuration and state of one channel."""
    _fields_ = ([(n, C.c_double) for n in ("acqfreq", "f_if", "foffset", "f_cf", "crate", "ctime")] +
                [(n, C.c_double * 2) for n in ("pllaw", "pllw2", "fllw", "dllaw", "dllw2")] +
                [(n, C.c_int) for n in ("ne", "nl", "loopms", "rate", "flagsync", "synci", "navcnt", "swloop")] +
                [("cnt", C.c_uint64)] +
                [(n, C.c_double) for n in ("carrNco", "codeNco", "carrErr", "codeErr", "freqErr")] +
                [(n, C.c_double * MAXTAPS) for n in ("II", "QQ", "oldI", "oldQ", "sumI", "sumQ", "oldsumI", "oldsumQ")] +
                [(n, C.c_int) for n in ("prn", "biti", "bit", "swsync", "swreset", "flagpol")] +
                [("bitIP", C.c_double), ("bitsync", C.c_int * 20)])


class TrkLog(C.Structure):
    """gnsscorr_trklog_t: one row per code period of a closed-loop run."""
    _fields_ = ([(n, C.c_double) for n in ("carrfreq", "codefreq", "carrErr", "codeErr", "carrNco", "codeNco", "freqErr",
                                            "remcode", "remcarr")] +
                [("buffloc", C.c_uint64), ("currnsamp", C.c_int), ("flagloopfilter", C.c_int), ("flagsync", C.c_int),
                 ("navbit", C.c_int)])


class ObsState(C.Structure):
    """gnsscorr_obs_t: what setobsdata() carries from call to call (ref src/sdrtrk.c:160-209)."""
    _fields_ = ([(n, C.c_double) for n in ("f_sf", "f_if", "foffset", "ctime")] + [("loopms", C.c_int)] +
                [("flagsyncf", C.c_int), ("polarity", C.c_int), ("firstsftow", C.c_double), ("firstsfcnt", C.c_uint64)] +
                [(n, C.c_double) for n in ("L", "Isum", "sumI0", "oldremcode")] +
                [("flagremcarradd", C.c_int), ("flagpolarityadd", C.c_int), ("loopcnt", C.c_uint64)])


class ObsRow(C.Structure):
    """gnsscorr_obsrow_t: element [0] of the observable histories after one call of setobsdata()."""
    _fields_ = ([(n, C.c_double) for n in ("tow", "remcout", "L", "D", "S")] + [("codei", C.c_uint64), ("cntout", C.c_uint64),
                ("snr", C.c_int), ("pad", C.c_int)])


def obs_replay(state, log_rows, II0, cnt0=0):
    """setobsdata() over one channel's log rows (numpy array of TrkLog) and its per-period trk.II[0]: returns the rows
    of observables (numpy array of ObsRow); `state` (ObsState) is updated.  Host code only."""
    L = lib()
    L.gnsscorr_obs_replay.restype = C.c_int
    L.gnsscorr_obs_replay.argtypes = [C.POINTER(ObsState), C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_int]
    log_rows = np.ascontiguousarray(log_rows)
    II0 = np.ascontiguousarray(II0, dtype=np.float64)
    n = int(log_rows.shape[0])
    out = np.zeros(max(n, 1), dtype=np.dtype(ObsRow))
    k = L.gnsscorr_obs_replay(C.byref(state), log_rows.ctypes.data, II0.ctypes.data, n, int(cnt0), out.ctypes.data, n)
    if k < 0:
        raise RuntimeError("gnsscorr_obs_replay: error %d" % k)
    return out[:k]


class FrameState(C.Structure):
    """gnsscorr_frame_t: frame synchronisation of L1 C/A on the decided nav bits (ref src/sdrnav.c:41-82)."""
    _fields_ = ([("fbits", C.c_int * 302)] + [(n, C.c_int) for n in ("polarity", "flagsyncf", "flagtow", "flagdec", "sfid", "pad")] +
                [("firstsf", C.c_uint64), ("firstsfcnt", C.c_uint64), ("firstsftow", C.c_double), ("tow_gpst", C.c_double)])


def frame_replay(state, log_rows, cnt0=0):
    """The nav bits of one channel's log rows through the preamble search / parity check / hand-over word; `state`
    (FrameState) is updated.  Host code only."""
    L = lib()
    L.gnsscorr_frame_replay.restype = C.c_int
    L.gnsscorr_frame_replay.argtypes = [C.POINTER(FrameState), C.c_void_p, C.c_int, C.c_uint64]
    log_rows = np.ascontiguousarray(log_rows)
    rc = L.gnsscorr_frame_replay(C.byref(state), log_rows.ctypes.data, int(log_rows.shape[0]), int(cnt0))
    if rc:
        raise RuntimeError("gnsscorr_frame_replay: error %d" % rc)


class G1FrameState(C.Structure):
    """gnsscorr_g1frame_t: frame synchronisation of GLONASS G1 on the decided symbols (ref src/sdrnav.c:40-82,
    src/sdrnav_glo.c)."""
    _fields_ = ([("fbits", C.c_int * 200)] +
                [(n, C.c_int) for n in ("polarity", "flagsyncf", "flagtow", "flagdec", "id", "ephcnt", "s1cnt")] +
                [("tk", C.c_int * 3)] + [(n, C.c_int) for n in ("nt", "slot", "n4", "iode", "update", "week")] +
                [("str", C.c_ubyte * 11), ("pad", C.c_ubyte * 5),
                 ("firstsf", C.c_uint64), ("firstsfcnt", C.c_uint64), ("firstsftow", C.c_double), ("tow_gpst", C.c_double)])


def g1frame_replay(state, log_rows, cnt0=0):
    """The symbols of one G1 channel's log rows through the time-mark search and the string decoder; `state`
    (G1FrameState) is updated.  Host code only; the caller sets state.ephcnt = 0 to let the time merge again."""
    L = lib()
    L.gnsscorr_g1frame_replay.restype = C.c_int
    L.gnsscorr_g1frame_replay.argtypes = [C.POINTER(G1FrameState), C.c_void_p, C.c_int, C.c_uint64]
    log_rows = np.ascontiguousarray(log_rows)
    rc = L.gnsscorr_g1frame_replay(C.byref(state), log_rows.ctypes.data, int(log_rows.shape[0]), int(cnt0))
    if rc:
        raise RuntimeError("gnsscorr_g1frame_replay: error %d" % rc)


OBSHIST, PTIMING, SYNCQCAP = 80, 68.802, 4096  # GNSSCORR_OBSHIST, GNSSCORR_PTIMING (ms), GNSSCORR_SYNCQCAP
EINVAL, ESTATE = -1, -3


class SyncFrame(C.Structure):
    """gnsscorr_syncframe_t: what a frame replay found, and the week, for the rows of one push."""
    _fields_ = [("flagdec", C.c_int), ("week", C.c_int), ("firstsf", C.c_uint64), ("firstsfcnt", C.c_uint64)]


class EpochObs(C.Structure):
    """gnsscorr_epochobs_t: one satellite's row of an observation epoch."""
    _fields_ = ([("ch", C.c_int), ("week", C.c_int)] + [(n, C.c_double) for n in ("tow", "P", "L", "D", "S")] +
                [("sampref", C.c_uint64)])


class Sync:
    """gnsscorr_sync_t: observation epochs from the rows of several channels (ref src/sdrsync.c:49-121; DESIGN.md
    section 3.8).  Host code only.  A refused call raises GnsscorrError with the code in `.code`."""

    def __init__(self, nch, outms):
        L = self._L = lib()
        L.gnsscorr_sync_last_error.restype = C.c_char_p
        L.gnsscorr_sync_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
        L.gnsscorr_sync_destroy.argtypes = [C.c_void_p]
        L.gnsscorr_sync_destroy.restype = None
        L.gnsscorr_sync_channel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]
        L.gnsscorr_sync_push.argtypes = [C.c_void_p, C.c_int, C.POINTER(SyncFrame), C.c_void_p, C.c_int]
        L.gnsscorr_sync_detach.argtypes = [C.c_void_p, C.c_int]
        L.gnsscorr_sync_flush.argtypes = [C.c_void_p]
        L.gnsscorr_sync_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self.h = C.c_void_p()
        self.nch = int(nch)
        self._ok(L.gnsscorr_sync_create(C.byref(self.h), int(nch), int(outms)))

    def _ok(self, rc):
        if rc < 0:
            e = GnsscorrError(self._L.gnsscorr_sync_last_error().decode())
            e.code = rc
            raise e
        return rc

    def close(self):
        if self.h:
            self._L.gnsscorr_sync_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def channel(self, ch, nsamp, ctime, ti):
        self._ok(self._L.gnsscorr_sync_channel(self.h, int(ch), int(nsamp), float(ctime), float(ti)))

    def push(self, ch, frame, rows):
        """rows: numpy array of ObsRow (obs_replay's); frame: SyncFrame, or a frame state plus week as (state, week)."""
        if isinstance(frame, tuple):
            frame = SyncFrame(int(frame[0].flagdec), int(frame[1]), int(frame[0].firstsf), int(frame[0].firstsfcnt))
        rows = np.ascontiguousarray(rows, dtype=np.dtype(ObsRow))
        self._ok(self._L.gnsscorr_sync_push(self.h, int(ch), C.byref(frame), rows.ctypes.data, int(rows.shape[0])))

    def detach(self, ch):
        self._ok(self._L.gnsscorr_sync_detach(self.h, int(ch)))

    def flush(self):
        self._ok(self._L.gnsscorr_sync_flush(self.h))

    def fetch(self, max_out=None):
        """The rows of the epochs made so far (numpy array of EpochObs); all of them without max_out."""
        parts = []
        while True:
            want = 1024 if max_out is None else max_out - sum(len(p) for p in parts)
            out = np.zeros(max(want, 1), dtype=np.dtype(EpochObs))
            k = self._ok(self._L.gnsscorr_sync_fetch(self.h, out.ctypes.data, want))
            parts.append(out[:k])
            if k < want or max_out is not None:
                return np.concatenate(parts)


class SbasFrameState(C.Structure):
    """gnsscorr_sbasframe_t: frame synchronisation of SBAS L1 on the decided symbols (ref src/sdrnav.c:40-82)."""
    _fields_ = ([("fbits", C.c_int * 1512)] +
                [(n, C.c_int) for n in ("polarity", "flagsyncf", "flagtow", "flagdec", "flagpol", "id", "week", "pad")] +
                [("firstsf", C.c_uint64), ("firstsfcnt", C.c_uint64), ("firstsftow", C.c_double), ("tow_gpst", C.c_double),
                 ("tow", C.c_double), ("msg", C.c_ubyte * 32)])


V27POLYA, V27POLYB = 0x6d, 0x4f              # libfec's fec.h (ref src/sdrinit.c:502)


class RxNavCh(C.Structure):
    """gnsscorr_rxnavch_t: the constants of one channel of an RxNav."""
    _fields_ = ([(n, C.c_int) for n in ("ctype", "nsamp", "loopms", "pad")] +
                [(n, C.c_double) for n in ("f_sf", "f_if", "foffset", "ctime", "ti", "oldremcode")])


class RxNavStat(C.Structure):
    """gnsscorr_rxnavstat_t: one channel's nav state in short."""
    _fields_ = ([(n, C.c_int) for n in ("ctype", "attached", "flagsyncf", "flagdec", "polarity", "week", "id", "resets")] +
                [(n, C.c_uint64) for n in ("cnt", "firstsf", "firstsfcnt", "nrows")] +
                [("firstsftow", C.c_double), ("tow", C.c_double)])


class RxNav:
    """gnsscorr_rxnav_t: frames, observables and epochs behind every step.  RxNav(channels, outms,
    hold_steps) creates one from RxNavCh's (or dicts of their fields); Engine.rx_nav() wraps the context's, which the
    context owns.  A refused call raises GnsscorrError with the code in `.code`."""

    def __init__(self, channels=None, outms=10, hold_steps=0, handle=None):
        L = self._L = lib()
        _bind_rxnav(L)
        self.own = handle is None
        if handle is not None:
            self.h = C.c_void_p(handle)
            return
        chans = [c if isinstance(c, RxNavCh) else RxNavCh(**c) for c in channels]
        arr = (RxNavCh * max(len(chans), 1))(*chans)
        self.h = C.c_void_p()
        self._ok(L.gnsscorr_rxnav_create(C.byref(self.h), len(chans), arr, int(outms), int(hold_steps)))

    def _ok(self, rc):
        if rc < 0:
            e = GnsscorrError(self._L.gnsscorr_rxnav_last_error().decode())
            e.code = rc
            raise e
        return rc

    def close(self):
        if self.h and self.own:
            self._L.gnsscorr_rxnav_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def week(self, ch, week):
        self._ok(self._L.gnsscorr_rxnav_week(self.h, int(ch), int(week)))

    def feed(self, log, II0, ndone, cnt_after, tracking, ctx=None):
        """log [nch][stride] of TrkLog, II0 [nch][stride], ndone / cnt_after / tracking [nch]; ctx: an Engine, for SBAS."""
        log = np.ascontiguousarray(log, dtype=np.dtype(TrkLog))
        II0 = np.ascontiguousarray(II0, dtype=np.float64)
        if log.ndim != 2 or II0.shape != log.shape:
            raise ValueError("RxNav.feed: log and II0 are [nch][stride]")
        ndone = np.ascontiguousarray(ndone, dtype=np.int32)
        cnt_after = np.ascontiguousarray(cnt_after, dtype=np.uint64)
        tracking = np.ascontiguousarray(tracking, dtype=np.int32)
        if not ndone.shape == cnt_after.shape == tracking.shape == (log.shape[0],):
            raise ValueError("RxNav.feed: ndone, cnt_after and tracking are [nch]")
        self._ok(self._L.gnsscorr_rxnav_feed(self.h, ctx.h if ctx is not None else None, log.ctypes.data, II0.ctypes.data,
                                             int(log.shape[1]), ndone.ctypes.data, cnt_after.ctypes.data, tracking.ctypes.data))

    def flush(self):
        self._ok(self._L.gnsscorr_rxnav_flush(self.h))

    def fetch(self, max_out=None):
        """The rows of the epochs made so far (numpy array of EpochObs); all of them without max_out."""
        parts = []
        while True:
            want = 1024 if max_out is None else max_out - sum(len(p) for p in parts)
            out = np.zeros(max(want, 1), dtype=np.dtype(EpochObs))
            k = self._ok(self._L.gnsscorr_rxnav_fetch(self.h, out.ctypes.data, want))
            parts.append(out[:k])
            if k < want or max_out is not None:
                return np.concatenate(parts)

    def status(self, nch):
        """numpy array [nch] of RxNavStat."""
        st = np.zeros(nch, dtype=np.dtype(RxNavStat))
        self._ok(self._L.gnsscorr_rxnav_status(self.h, st.ctypes.data))
        return st

    def frame(self, ch, ctype):
        """A copy of channel ch's frame state: FrameState, SbasFrameState or G1FrameState by `ctype`."""
        st = {CTYPE_L1CA: FrameState, CTYPE_L1SBAS: SbasFrameState, CTYPE_G1: G1FrameState}[ctype]()
        self._ok(self._L.gnsscorr_rxnav_frame(self.h, int(ch), C.byref(st), C.sizeof(st)))
        return st

    def rows(self, ch, max_rows=4096):
        """The rows of observables the last feed made for channel ch (numpy array of ObsRow)."""
        out = np.zeros(max(max_rows, 1), dtype=np.dtype(ObsRow))
        k = self._ok(self._L.gnsscorr_rxnav_rows(self.h, int(ch), out.ctypes.data, int(max_rows)))
        return out[:k]


def _bind_rxnav(L):
    L.gnsscorr_rxnav_last_error.restype = C.c_char_p
    L.gnsscorr_rxnav_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(RxNavCh), C.c_int, C.c_int]
    L.gnsscorr_rxnav_destroy.argtypes = [C.c_void_p]
    L.gnsscorr_rxnav_destroy.restype = None
    L.gnsscorr_rxnav_week.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.gnsscorr_rxnav_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gnsscorr_rxnav_flush.argtypes = [C.c_void_p]
    L.gnsscorr_rxnav_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.gnsscorr_rxnav_status.argtypes = [C.c_void_p, C.c_void_p]
    L.gnsscorr_rxnav_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.gnsscorr_rxnav_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.gnsscorr_rx_nav_start.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.gnsscorr_rx_nav_step.argtypes = [C.c_void_p, C.c_int]
    L.gnsscorr_rx_nav_stop.argtypes = [C.c_void_p]
    L.gnsscorr_rx_nav.argtypes = [C.c_void_p]
    L.gnsscorr_rx_nav.restype = C.c_void_p
    L.gnsscorr_trk_fetch_prompt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]


class SpecParams(C.Structure):
    """gnsscorr_spec_t: one IF-monitor configuration (include/gnsscorr.h)."""
    _fields_ = [("ftype", C.c_int), ("nfft", C.c_int), ("nloop", C.c_int), ("n", C.c_int), ("f_sf", C.c_double)]


SPEC_HIST = 9          # counts per row of gnsscorr_spec_fetch's hist: bins -7,-5,...,+7 and d == maxd > 7
SPEC_NLOOP = 100       # ref src/sdr.h:232


class AcqRes(C.Structure):
    _fields_ = [("acqcodei", C.c_int), ("freqi", C.c_int), ("acqfreq", C.c_double),
                ("cn0", C.c_double), ("peakr", C.c_double), ("flagacq", C.c_int),
                ("iters", C.c_int), ("buffloc", C.c_uint64)]


class AcqFine(C.Structure):
    """gnsscorr_acqfine_t: the refined carrier frequency of one channel (gnsscorr_acq_fetch_fine)."""
    _fields_ = [("finefreq", C.c_double), ("quality", C.c_double), ("q", C.c_int), ("nref", C.c_int)]


CH_IDLE, CH_SEARCH, CH_TRACK = 0, 1, 2
ACQSLEEP = 2000                              # ms, ref src/sdr.h:149


class RxStat(C.Structure):
    """gnsscorr_rxstat_t: one channel of the receiver schedule (gnsscorr_rx_status)."""
    _fields_ = [("state", C.c_int), ("attempts", C.c_int), ("next_try", C.c_uint64), ("acq_wrpos", C.c_uint64),
                ("acq", AcqRes), ("cnt", C.c_uint64)]


class LockPrm(C.Structure):
    """gnsscorr_lockprm_t: the lock monitor's parameters (kbits 0: off)."""
    _fields_ = [("sync_periods", C.c_int), ("kbits", C.c_int), ("nbad", C.c_int), ("pad", C.c_int), ("mu_min", C.c_double)]


class LockState(C.Structure):
    """gnsscorr_lock_t: the lock detector's state of one channel."""
    _fields_ = ([(n, C.c_double) for n in ("sI", "sQ", "w", "npsum", "mu_last")] + [("lost_cnt", C.c_uint64)] +
                [(n, C.c_int) for n in ("open", "n", "k", "nbad", "lost", "reason", "windows", "pad")])


class BsyncPrm(C.Structure):
    """gnsscorr_bsyncprm_t: the parameters of bit synchronisation by symbol energy (nsym 0: off).  Tests of the best
    alignment against the one half a symbol away come every nsym whole symbols from start_cnt on, up to nsym_max; a
    test passes when E[best] >= gate * E[half]."""
    _fields_ = [("start_cnt", C.c_int), ("nsym", C.c_int), ("nsym_max", C.c_int), ("pad", C.c_int), ("gate", C.c_double)]


class BsyncState(C.Structure):
    """gnsscorr_bsync_t: the bit-synchronisation detector's state of one channel.  Per offset o (a
    symbol begins on the periods with cnt mod rate == o): E the energy of the whole symbols so far, sI / sQ / fill the
    open symbol.  a0: cnt of the first counted row (armed); n: whole symbols per offset; done: 0 running, 1 decided
    (best, synci = the biti of a symbol's last period, decided_cnt, ratio_last), 2 given up at nsym_max, 3 the loop
    synchronised first."""
    _fields_ = ([("E", C.c_double * 20), ("sI", C.c_double * 20), ("sQ", C.c_double * 20), ("ratio_last", C.c_double),
                 ("a0", C.c_uint64), ("decided_cnt", C.c_uint64), ("fill", C.c_int * 20)] +
                [(n, C.c_int) for n in ("armed", "n", "tests", "done", "best", "synci")])


class CfmPrm(C.Structure):
    """gnsscorr_cfmprm_t: the parameters of the correlation monitor (kbits 0: off).  Windows of kbits whole nav bits
    behind the first skip_bits; a window is bad when its prompt sum is not positive or a pair j <= npair has
    |delta - dref| > dtol or |ratio - rref| > rtol; nbad bad windows in a row raise the alarm."""
    _fields_ = [("kbits", C.c_int), ("skip_bits", C.c_int), ("nbad", C.c_int), ("npair", C.c_int), ("dtol", C.c_double),
                ("rtol", C.c_double), ("dref", C.c_double * 16), ("rref", C.c_double * 16)]


class CfmState(C.Structure):
    """gnsscorr_cfm_t: the correlation monitor's state of one channel.  Per tap t (P, E1, L1, E2, L2,
    ...): sI / sQ the open bit, aI / aQ / aP the open window (data-wiped sums and power), cfI / cfQ / cfP the last
    closed window; per pair j: delta[j-1], ratio[j-1] of that window.  win_cnt: cnt of the period that closed it; bits:
    whole bits seen; nbad: bad windows in a row; alarm, alarms, windows, worst_pair (the first failing pair, 0 none)."""
    _fields_ = ([(n, C.c_double * 33) for n in ("sI", "sQ", "aI", "aQ", "aP", "cfI", "cfQ", "cfP")] +
                [("delta", C.c_double * 16), ("ratio", C.c_double * 16), ("win_cnt", C.c_uint64)] +
                [(n, C.c_int) for n in ("open", "n", "k", "bits", "nbad", "alarm", "alarms", "windows", "worst_pair", "pad")])


def cfm_prm(kbits=0, skip_bits=0, nbad=1, npair=1, dtol=0.0, rtol=0.0, dref=(), rref=()):
    """A CfmPrm from plain values; dref / rref shorter than 16 are filled with 0."""
    p = CfmPrm(kbits=kbits, skip_bits=skip_bits, nbad=nbad, npair=npair, dtol=dtol, rtol=rtol)
    for j, v in enumerate(dref):
        p.dref[j] = v
    for j, v in enumerate(rref):
        p.rref[j] = v
    return p


def mu_from_cn0(cn0_dbhz, rate, ctime):
    """The mean narrow-band / wide-band power ratio of a nav bit of `rate` periods of `ctime` seconds at that C/N0:
    (1 + rate*x) / (1 + x) with x = 10^(cn0/10) * ctime, the inverse of C/N0 = (mu - 1) / ((rate - mu) * ctime).  For
    callers who think of the monitor's mu_min in dB-Hz; the tracker biases the measured mu low."""
    x = 10.0 ** (cn0_dbhz / 10.0) * ctime
    return (1.0 + rate * x) / (1.0 + x)


# ---- ctypes mirrors of include/sdr_compat.h (ref src/sdr.h:344-511) --------
OBSINTERPN = 80


class SdrAcq(C.Structure):
    _fields_ = [("intg", C.c_int), ("hband", C.c_double), ("step", C.c_double), ("nfreq", C.c_int),
                ("freq", C.POINTER(C.c_double)), ("acqcodei", C.c_int), ("freqi", C.c_int),
                ("acqfreq", C.c_double), ("nfft", C.c_int), ("cn0", C.c_double), ("peakr", C.c_double)]


class SdrTrkPrm(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("pllb", "dllb", "fllb", "dllw2", "dllaw", "pllw2", "pllaw", "fllw")]


class SdrTrk(C.Structure):
    _fields_ = ([(n, C.c_double) for n in ("codefreq", "carrfreq", "remcode", "remcarr", "oldremcode",
                                            "oldremcarr", "codeNco", "codeErr", "carrNco", "carrErr",
                                            "freqErr")] +
                [("buffloc", C.c_uint64), ("tow", C.c_double * OBSINTERPN),
                 ("codei", C.c_uint64 * OBSINTERPN), ("codeisum", C.c_uint64 * OBSINTERPN),
                 ("cntout", C.c_uint64 * OBSINTERPN), ("remcout", C.c_double * OBSINTERPN),
                 ("L", C.c_double * OBSINTERPN), ("D", C.c_double * OBSINTERPN),
                 ("S", C.c_double * OBSINTERPN)] +
                [(n, C.POINTER(C.c_double)) for n in ("II", "QQ", "oldI", "oldQ", "sumI", "sumQ",
                                                      "oldsumI", "oldsumQ")] +
                [("Isum", C.c_double), ("loop", C.c_int), ("loopms", C.c_int),
                 ("flagpolarityadd", C.c_int), ("flagremcarradd", C.c_int), ("flagloopfilter", C.c_int),
                 ("corrn", C.c_int), ("corrp", C.POINTER(C.c_int)), ("corrx", C.POINTER(C.c_double)),
                 ("ne", C.c_int), ("nl", C.c_int), ("prm1", SdrTrkPrm), ("prm2", SdrTrkPrm)])


class SdrCh(C.Structure):
    _fields_ = [("hsdr", C.c_ulong), ("no", C.c_int), ("sat", C.c_int), ("sys", C.c_int), ("prn", C.c_int),
                ("satstr", C.c_char * 5), ("ctype", C.c_int), ("dtype", C.c_int), ("ftype", C.c_int),
                ("f_cf", C.c_double), ("f_sf", C.c_double), ("f_if", C.c_double), ("foffset", C.c_double),
                ("code", C.POINTER(C.c_short)), ("xcode", C.c_void_p), ("clen", C.c_int),
                ("crate", C.c_double), ("ctime", C.c_double), ("ti", C.c_double), ("ci", C.c_double),
                ("nsamp", C.c_int), ("currnsamp", C.c_int), ("nsampchip", C.c_int),
                ("acq", SdrAcq), ("trk", SdrTrk), ("nav", C.c_byte * 1008),
                ("flagacq", C.c_int), ("flagtrk", C.c_int)]


class SdrIni(C.Structure):
    _fields_ = [("fend", C.c_int), ("f_cf", C.c_double * 2), ("f_sf", C.c_double * 2),
                ("f_if", C.c_double * 2), ("dtype", C.c_int * 2), ("fp1", C.c_void_p), ("fp2", C.c_void_p),
                ("file1", C.c_char * 1024), ("file2", C.c_char * 1024), ("useif1", C.c_int),
                ("useif2", C.c_int), ("nch", C.c_int), ("nchL1", C.c_int), ("nchL2", C.c_int),
                ("nchL5", C.c_int), ("nchL6", C.c_int), ("prn", C.c_int * 55), ("sys", C.c_int * 55),
                ("ctype", C.c_int * 55), ("ftype", C.c_int * 55), ("pltacq", C.c_int), ("plttrk", C.c_int),
                ("pltspec", C.c_int), ("outms", C.c_int), ("rinex", C.c_int), ("rtcm", C.c_int),
                ("sbas", C.c_int), ("log", C.c_int), ("rinexpath", C.c_char * 1024), ("rtcmport", C.c_int),
                ("sbasport", C.c_int), ("trkcorrn", C.c_int), ("trkcorrd", C.c_int), ("trkcorrp", C.c_int),
                ("trkdllb", C.c_double * 2), ("trkpllb", C.c_double * 2), ("trkfllb", C.c_double * 2),
                ("rtlsdrppmerr", C.c_int)]


class SdrStat(C.Structure):
    _fields_ = [("stopflag", C.c_int), ("specflag", C.c_int), ("buffsize", C.c_int),
                ("fendbuffsize", C.c_int), ("buff", C.c_void_p), ("buff2", C.c_void_p),
                ("tmpbuff", C.c_void_p), ("buffcnt", C.c_uint64)]


_lib = None
_KEEP = object()

# every symbol include/gnsscorr.h and include/sdr_compat.h declare and the library defines
EXPORTS_GNSSCORR = [
    "gnsscorr_last_error", "gnsscorr_device_count", "gnsscorr_create", "gnsscorr_destroy",
    "gnsscorr_stream", "gnsscorr_sync", "gnsscorr_ring_create", "gnsscorr_ring_push",
    "gnsscorr_ring_commit", "gnsscorr_ring_wrpos", "gnsscorr_ring_devptr", "gnsscorr_set_channels",
    "gnsscorr_num_channels", "gnsscorr_trk_set_state", "gnsscorr_trk_get_state", "gnsscorr_trk_run",
    "gnsscorr_trk_fetch", "gnsscorr_trk_fetch_sums", "gnsscorr_trk_devptrs", "gnsscorr_acq_run",
    "gnsscorr_acq_fetch", "gnsscorr_trk_start_from_acq", "gnsscorr_acq_power", "gnsscorr_fft16k", "gnsscorr_pspec",
    "gnsscorr_timing_enable", "gnsscorr_timing_read", "gnsscorr_timing_reset", "gnsscorr_default_ctx",
    "gnsscorr_spec_run", "gnsscorr_spec_fetch", "gnsscorr_trk_loop_lapped",
    "gnsscorr_acq_run_subset", "gnsscorr_loop_start_from_acq", "gnsscorr_rx_start", "gnsscorr_rx_set",
    "gnsscorr_rx_step", "gnsscorr_rx_status", "gnsscorr_fec_run", "gnsscorr_sbasframe_replay",
    "gnsscorr_lock_run", "gnsscorr_rx_lock_set", "gnsscorr_rx_lock_status",
    "gnsscorr_bsync_run", "gnsscorr_rx_bsync_set", "gnsscorr_rx_bsync_status",
    "gnsscorr_cfm_run", "gnsscorr_rx_cfm_set", "gnsscorr_rx_cfm_status",
    "gnsscorr_acq_set_coherent", "gnsscorr_acq_get_coherent", "gnsscorr_g1frame_replay",
    "gnsscorr_acq_set_bitedge", "gnsscorr_acq_get_bitedge", "gnsscorr_acq_fetch_edge",
    "gnsscorr_acq_set_refine", "gnsscorr_acq_get_refine", "gnsscorr_acq_fetch_fine",
    "gnsscorr_acq_set_codedoppler", "gnsscorr_acq_get_codedoppler", "gnsscorr_acq_fetch_shifts",
    "gnsscorr_sync_create", "gnsscorr_sync_destroy", "gnsscorr_sync_channel", "gnsscorr_sync_push",
    "gnsscorr_sync_detach", "gnsscorr_sync_flush", "gnsscorr_sync_fetch", "gnsscorr_sync_last_error",
    "gnsscorr_trk_fetch_prompt", "gnsscorr_rxnav_create", "gnsscorr_rxnav_destroy", "gnsscorr_rxnav_week",
    "gnsscorr_rxnav_feed", "gnsscorr_rxnav_flush", "gnsscorr_rxnav_fetch", "gnsscorr_rxnav_status", "gnsscorr_rxnav_frame",
    "gnsscorr_rxnav_rows", "gnsscorr_rxnav_last_error", "gnsscorr_rx_nav_start", "gnsscorr_rx_nav_step", "gnsscorr_rx_nav",
    "gnsscorr_rx_nav_stop"]
EXPORTS_SDR = [
    "sdracquisition", "checkacquisition", "sdrtracking", "cumsumcorr", "clearcumsumcorr", "pll", "dll",
    "readinifile", "chk_initvalue", "initacqstruct", "inittrkprmstruct", "inittrkstruct", "initsdrch",
    "freesdrch", "cpxcpx", "cpxfft", "cpxifft", "cpxconv", "cpxpspec", "mixcarr", "rescode", "pcorrelator", "correlator",
    "maxvd", "meanvd", "ind2sub", "gencode", "rcvgetbuff", "file_pushtomembuf", "file_getbuff",
    "sdrnavigation", "sdrini", "sdrstat", "hbuffmtx", "hreadmtx", "hfftmtx", "hobsmtx",
    "hanning", "calchistgram", "spectrumanalyzer"]


def lib():
    """The loaded libgnsscorr.so; raises GnsscorrError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GnsscorrError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    L.gnsscorr_last_error.restype = C.c_char_p
    L.gnsscorr_stream.restype = C.c_void_p
    L.gnsscorr_stream.argtypes = [C.c_void_p]
    L.gnsscorr_ring_wrpos.restype = C.c_uint64
    L.gnsscorr_ring_wrpos.argtypes = [C.c_void_p, C.c_int]
    L.gnsscorr_ring_devptr.restype = C.c_void_p
    L.gnsscorr_ring_devptr.argtypes = [C.c_void_p, C.c_int]
    L.gnsscorr_default_ctx.restype = C.c_void_p
    L.gnsscorr_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p]
    L.gnsscorr_destroy.argtypes = [C.c_void_p]
    L.gnsscorr_destroy.restype = None
    L.gnsscorr_sync.argtypes = [C.c_void_p]
    L.gnsscorr_ring_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p]
    L.gnsscorr_ring_push.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
    L.gnsscorr_ring_commit.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    L.gnsscorr_ring_push_packed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
    L.gnsscorr_ring_read.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_void_p]
    L.gnsscorr_set_channels.argtypes = [C.c_void_p, C.c_int, C.POINTER(ChanDesc)]
    L.gnsscorr_num_channels.argtypes = [C.c_void_p]
    L.gnsscorr_trk_set_state.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(TrkState)]
    L.gnsscorr_trk_get_state.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(TrkState)]
    L.gnsscorr_trk_run.argtypes = [C.c_void_p, C.c_int]
    L.gnsscorr_trk_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gnsscorr_trk_fetch_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.gnsscorr_trk_devptrs.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.gnsscorr_loop_set.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(LoopState)]
    L.gnsscorr_loop_get.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(LoopState)]
    L.gnsscorr_trk_run_loop.argtypes = [C.c_void_p, C.c_int]
    L.gnsscorr_trk_fetch_log.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.gnsscorr_trk_loop_lapped.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.gnsscorr_acq_run.argtypes = [C.c_void_p, C.c_uint64]
    L.gnsscorr_acq_run_subset.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int), C.c_int]
    L.gnsscorr_acq_fetch.argtypes = [C.c_void_p, C.POINTER(AcqRes)]
    L.gnsscorr_loop_start_from_acq.argtypes = [C.c_void_p]
    L.gnsscorr_rx_start.argtypes = [C.c_void_p, C.c_int]
    L.gnsscorr_rx_set.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.gnsscorr_rx_step.argtypes = [C.c_void_p, C.c_int]
    L.gnsscorr_rx_status.argtypes = [C.c_void_p, C.POINTER(RxStat)]
    L.gnsscorr_trk_start_from_acq.argtypes = [C.c_void_p]
    L.gnsscorr_acq_power.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "gnsscorr_acq_set_coherent"):     # (absent from an A/B library built before it: tools/acq_coh_time.py)
        L.gnsscorr_acq_set_coherent.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.gnsscorr_acq_get_coherent.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    if hasattr(L, "gnsscorr_acq_set_bitedge"):      # (likewise: tools/acq_edge_time.py)
        L.gnsscorr_acq_set_bitedge.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.gnsscorr_acq_get_bitedge.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.gnsscorr_acq_fetch_edge.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    if hasattr(L, "gnsscorr_acq_set_refine"):       # (likewise: tools/acq_fine_time.py)
        L.gnsscorr_acq_set_refine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.gnsscorr_acq_get_refine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.gnsscorr_acq_fetch_fine.argtypes = [C.c_void_p, C.POINTER(AcqFine), C.c_void_p]
    if hasattr(L, "gnsscorr_acq_set_codedoppler"):  # (likewise: tools/acq_slip_time.py)
        L.gnsscorr_acq_set_codedoppler.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.gnsscorr_acq_get_codedoppler.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.gnsscorr_acq_fetch_shifts.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    if hasattr(L, "gnsscorr_rxnav_create"):         # (likewise: tools/rx_nav_time.py)
        _bind_rxnav(L)
    L.gnsscorr_fft16k.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.gnsscorr_pspec.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.gnsscorr_timing_enable.argtypes = [C.c_void_p, C.c_int]
    L.gnsscorr_timing_reset.argtypes = [C.c_void_p]
    L.gnsscorr_timing_read.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.gnsscorr_spec_run.argtypes = [C.c_void_p, C.POINTER(SpecParams), C.c_int, C.c_void_p, C.c_void_p]
    L.gnsscorr_spec_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                      C.c_size_t, C.c_void_p, C.c_size_t]
    L.gnsscorr_fec_run.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 9 + [C.c_void_p, C.c_int]
    L.gnsscorr_sbasframe_replay.argtypes = [C.c_void_p, C.POINTER(SbasFrameState), C.c_void_p, C.c_int, C.c_uint64,
                                            C.c_void_p, C.c_int]
    L.gnsscorr_lock_run.argtypes = [C.c_void_p] + [C.c_void_p] * 8 + [C.c_int, C.c_int]
    L.gnsscorr_rx_lock_set.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(LockPrm)]
    L.gnsscorr_rx_lock_status.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.gnsscorr_bsync_run.argtypes = [C.c_void_p] + [C.c_void_p] * 8 + [C.c_int, C.c_int]
    L.gnsscorr_rx_bsync_set.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(BsyncPrm)]
    L.gnsscorr_rx_bsync_status.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.gnsscorr_cfm_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int]
    L.gnsscorr_rx_cfm_set.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(CfmPrm)]
    L.gnsscorr_rx_cfm_status.argtypes = [C.c_void_p, C.c_void_p]
    L.gnsscorr_debug_fec_parts.argtypes = [C.c_void_p, C.c_int]   # (tools; not part of include/gnsscorr.h)
    L.gnsscorr_debug_poison.argtypes = [C.c_void_p, C.c_int]      # (tests; not part of include/gnsscorr.h)
    if hasattr(L, "gnsscorr_debug_cmb_stats"):                    # (tests; bound when present, like the symbols below)
        L.gnsscorr_debug_cmb_stats.argtypes = [C.c_void_p]
        L.gnsscorr_debug_cmb_stats.restype = None
    # reference-named symbols (bound when present; tests/test_abi.py checks that all are)
    def _sig(name, restype, argtypes):
        try:
            f = getattr(L, name)
        except AttributeError:
            return
        if restype is not _KEEP:
            f.restype = restype
        f.argtypes = argtypes

    _sig("gencode", C.POINTER(C.c_short), [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)])
    _sig("initsdrch", _KEEP, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(SdrCh)])
    _sig("freesdrch", None, [C.POINTER(SdrCh)])
    _sig("sdrtracking", C.c_uint64, [C.POINTER(SdrCh), C.c_uint64, C.c_uint64])
    _sig("sdracquisition", C.c_uint64, [C.POINTER(SdrCh), C.c_void_p])
    _sig("checkacquisition", _KEEP, [C.c_void_p, C.POINTER(SdrCh)])
    _sig("correlator", None, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.c_int])
    _sig("pcorrelator", None, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p])
    _sig("cumsumcorr", None, [C.POINTER(SdrTrk), C.c_int])
    _sig("clearcumsumcorr", None, [C.POINTER(SdrTrk)])
    _sig("pll", None, [C.POINTER(SdrCh), C.POINTER(SdrTrkPrm), C.c_double])
    _sig("dll", None, [C.POINTER(SdrCh), C.POINTER(SdrTrkPrm), C.c_double])
    _sig("readinifile_at", _KEEP, [C.POINTER(SdrIni), C.c_char_p])
    _sig("rcvinit_file", _KEEP, [C.POINTER(SdrIni)])
    _sig("file_pushtomembuf", None, [])
    _sig("file_getbuff", None, [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p])
    _sig("rcvgetbuff", _KEEP, [C.POINTER(SdrIni), C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p])
    _sig("chk_initvalue", _KEEP, [C.POINTER(SdrIni)])
    _sig("cpxpspec", None, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p])
    _sig("cpxfft", None, [C.c_void_p, C.c_void_p, C.c_int])
    _sig("cpxifft", None, [C.c_void_p, C.c_void_p, C.c_int])
    _sig("cpxcpx", None, [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p])
    _sig("cpxconv", None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p])
    _sig("mixcarr", C.c_double, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p])
    _sig("rescode", C.c_double, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_void_p])
    _sig("maxvd", C.c_double, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)])
    _sig("meanvd", C.c_double, [C.c_void_p, C.c_int, C.c_int, C.c_int])
    _sig("hanning", None, [C.c_int, C.c_void_p])
    _sig("calchistgram", None, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    _sig("spectrumanalyzer", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p])
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise GnsscorrError(lib().gnsscorr_last_error().decode())


def sdrini():
    return SdrIni.in_dll(lib(), "sdrini")


def sdrstat():
    return SdrStat.in_dll(lib(), "sdrstat")


def cmb_stats():
    """(tests) sdrtracking()'s combiner so far: (launch chains, requests served, requests of the largest chain)."""
    out = (C.c_ulonglong * 3)()
    lib().gnsscorr_debug_cmb_stats(out)
    return tuple(out)


def gencode(prn, ctype):
    """gencode() of the library (ref src/sdrcode.c:523-539): (int16 chips, chip rate)."""
    n, cr = C.c_int(), C.c_double()
    p = lib().gencode(prn, ctype, C.byref(n), C.byref(cr))
    if not p:
        raise GnsscorrError(f"gencode failed for prn {prn} ctype {ctype}")
    code = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
    C.CDLL(None).free(p)
    return code, cr.value


def _samples(data, dtype):
    """int8 bytes of a sample block (n for dtype 1, (n, 2) or 2n interleaved for dtype 2) and n."""
    a = np.ascontiguousarray(data, dtype=np.int8).reshape(-1)
    if dtype not in (DTYPEI, DTYPEIQ) or a.size % dtype:
        raise ValueError(f"dtype {dtype} with {a.size} bytes")
    return a, a.size // dtype


def calchistgram(data, dtype):
    """calchistgram() of the library (ref src/sdrspec.c:170-206): (xI, yI, xQ, yQ), 8 bins each.  Host code."""
    a, n = _samples(data, dtype)
    xI, yI, xQ, yQ = (np.zeros(8) for _ in range(4))
    lib().calchistgram(a.ctypes.data, dtype, n, xI.ctypes.data, yI.ctypes.data, xQ.ctypes.data, yQ.ctypes.data)
    return xI, yI, xQ, yQ


def spectrumanalyzer(data, dtype, f_sf, nfft=16384):
    """spectrumanalyzer() of the library (ref src/sdrspec.c:232-296) on the default context's device: (freq MHz,
    pspec dB), dtype*nfft each.  Its 100 segment offsets come from the C library's rand(), as in the reference."""
    a, n = _samples(data, dtype)
    freq = np.zeros(dtype * nfft)
    pspec = np.zeros(dtype * nfft)
    if lib().spectrumanalyzer(a.ctypes.data, dtype, n, float(f_sf), nfft, freq.ctypes.data, pspec.ctypes.data) != 0:
        raise GnsscorrError(lib().gnsscorr_last_error().decode())
    return freq, pspec


def coherent_step(ncoh, ctime=1e-3, step=200):
    """The Doppler step (whole Hz) recommended for a search that integrates ncoh code periods of ctime seconds
    coherently: the reference's `step` (ACQSTEP), but no more than 1/(2*ncoh*ctime) -- 200 / 100 / 50 Hz for 1 / 5 / 10
    periods of 1 ms.  For Channel(hband=, step=coherent_step(ncoh), ncoh=ncoh)."""
    return max(1, min(int(step), int(1.0 / (2.0 * ncoh * ctime) + 1e-6)))


class Channel:
    """Constants of one receiver channel, derived exactly as initsdrch() does
    (ref src/sdrinit.c:583-657, acquisition grid :385-394,:633-635, taps :446-455).  fend / ppmerr stand for
    sdrini.fend / sdrini.rtlsdrppmerr: RTL-SDR file replay (FEND_FRTLSDR) offsets the channel by f_cf*ppmerr*1e-6.
    ncoh: code periods the search integrates coherently per group (gnsscorr_acq_set_coherent; 1: the reference's
    integration); estep: step of the bit-edge hypotheses of a group (gnsscorr_acq_set_bitedge; 0: none, otherwise
    1 .. ncoh-1 with ncoh >= 2); nref: code periods an acquired channel's carrier frequency is refined over
    (gnsscorr_acq_set_refine; 0: none, otherwise 2 .. min(intg, MAXCOH)); cdop: the search compensates code Doppler
    across its groups with the channel's own f_cf (gnsscorr_acq_set_codedoppler; for G1 the slot's carrier);
    Engine.set_channels applies them, in that order."""

    def __init__(self, prn, ctype=CTYPE_L1CA, dtype=DTYPEIQ, ftype=FTYPE1, f_cf=1575.42e6,
                 f_sf=16.368e6, f_if=0.0, corrn=2, corrd=3, corrp=3, hband=7000, step=200, intg=10,
                 fend=FEND_FILE, ppmerr=0, ncoh=1, estep=0, nref=0, cdop=False):
        self.prn, self.ctype, self.dtype, self.ftype = prn, ctype, dtype, ftype
        self.code, self.crate = gencode(prn, ctype)
        self.clen = len(self.code)
        self.f_sf, self.f_if = f_sf, f_if
        self.ti = 1 / f_sf
        self.ci = self.ti * self.crate
        self.ctime = self.clen / self.crate
        self.nsamp = int(f_sf * self.ctime)
        self.nsampchip = int(self.nsamp / self.clen)
        if ctype == CTYPE_G1:
            self.f_cf = 1.60200e9 + 0.56250e6 * prn
            self.foffset = 0.56250e6 * prn
        elif fend == FEND_FRTLSDR:
            self.f_cf, self.foffset = f_cf, f_cf * ppmerr * 1e-6
        else:
            self.f_cf, self.foffset = f_cf, 0.0
        self.intg = intg
        self.ncoh = ncoh
        self.estep = estep
        self.nref = nref
        self.cdop = bool(cdop)
        self.nfreq = 2 * (hband // step) + 1
        self.nfft = 2 * self.nsamp
        self.freq = np.array([f_if + ((i - (self.nfreq - 1) // 2) * float(step)) + self.foffset
                              for i in range(self.nfreq)], dtype=np.float64)
        self.corrn = corrn
        self.corrp = np.array([corrd * (i + 1) for i in range(corrn)], dtype=np.int32)
        self.ne = self.nl = 0
        for i in range(corrn):
            if self.corrp[i] == corrp:
                self.ne, self.nl = 2 * (i + 1) - 1, 2 * (i + 1)
        self.ntap = 1 + 2 * corrn

    def desc(self):
        d = ChanDesc()
        d.prn, d.ctype, d.dtype, d.ftype = self.prn, self.ctype, self.dtype, self.ftype
        d.clen, d.nsamp, d.nsampchip = self.clen, self.nsamp, self.nsampchip
        d.f_sf, d.f_if, d.foffset = self.f_sf, self.f_if, self.foffset
        d.crate, d.ctime, d.ti = self.crate, self.ctime, self.ti
        self._code16 = np.ascontiguousarray(self.code, dtype=np.int16)
        d.code = self._code16.ctypes.data_as(C.POINTER(C.c_short))
        d.intg, d.nfreq, d.nfft = self.intg, self.nfreq, self.nfft
        d.freq = self.freq.ctypes.data_as(C.POINTER(C.c_double))
        d.corrn = self.corrn
        d.corrp = self.corrp.ctypes.data_as(C.POINTER(C.c_int))
        return d


class Engine:
    """One GPU context of libgnsscorr (see include/gnsscorr.h for the semantics)."""

    def __init__(self, device=0, stream=None):
        self._L = lib()
        h = C.c_void_p()
        _check(self._L.gnsscorr_create(C.byref(h), device, stream))
        self.h = h
        self.channels = []

    def close(self):
        if self.h:
            self._L.gnsscorr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return self._L.gnsscorr_stream(self.h)

    def stream_ptr(self):
        """The context's HIP stream as an integer (for torch.cuda.ExternalStream)."""
        return int(self._L.gnsscorr_stream(self.h) or 0)

    def sync(self):
        _check(self._L.gnsscorr_sync(self.h))

    def debug_poison(self, byte):
        """(tests) Fill every device buffer the context allocates from now on with `byte` (0..255) before its
        first use, instead of whatever the memory held; -1: off (the default)."""
        _check(self._L.gnsscorr_debug_poison(self.h, byte))

    # -- ring
    def ring_create(self, ftype, dtype, ringlen, devptr=None):
        _check(self._L.gnsscorr_ring_create(self.h, ftype, dtype, ringlen, devptr))
        self._ring_dtype = getattr(self, "_ring_dtype", {})
        self._ring_dtype[ftype] = dtype

    def ring_push(self, ftype, samples):
        a = np.ascontiguousarray(samples, dtype=np.int8)
        dtype = 2 if (a.ndim == 2 and a.shape[1] == 2) else None
        n = a.shape[0] if dtype == 2 else a.size
        _check(self._L.gnsscorr_ring_push(self.h, ftype, a.ctypes.data, n))

    def ring_push_raw(self, ftype, raw_bytes, nsamp):
        a = np.ascontiguousarray(raw_bytes, dtype=np.int8)
        _check(self._L.gnsscorr_ring_push(self.h, ftype, a.ctypes.data, nsamp))

    def ring_push_packed(self, fmt, packed, nsamp):
        """fmt: FMT_STEREO (one byte per sample instant) or FMT_RTLSDR (2*nsamp unsigned bytes)"""
        a = np.ascontiguousarray(packed, dtype=np.uint8)
        _check(self._L.gnsscorr_ring_push_packed(self.h, fmt, a.ctypes.data, nsamp))

    def ring_read(self, ftype, buffloc, n, dtype):
        out = np.empty((n, 2) if dtype == 2 else (n,), np.int8)
        _check(self._L.gnsscorr_ring_read(self.h, ftype, buffloc, n, out.ctypes.data))
        return out

    def ring_commit(self, ftype, nsamp):
        _check(self._L.gnsscorr_ring_commit(self.h, ftype, nsamp))

    def ring_wrpos(self, ftype):
        return self._L.gnsscorr_ring_wrpos(self.h, ftype)

    def ring_devptr(self, ftype):
        return self._L.gnsscorr_ring_devptr(self.h, ftype)

    # -- channels
    def set_channels(self, channels):
        arr = (ChanDesc * len(channels))(*[c.desc() for c in channels])
        _check(self._L.gnsscorr_set_channels(self.h, len(channels), arr))
        self.channels = list(channels)
        ncoh = [getattr(c, "ncoh", 1) for c in channels]
        if any(k != 1 for k in ncoh):
            self.acq_set_coherent(ncoh)
        estep = [getattr(c, "estep", 0) for c in channels]
        if any(k != 0 for k in estep):
            self.acq_set_bitedge(estep)
        nref = [getattr(c, "nref", 0) for c in channels]
        if any(k != 0 for k in nref):
            self.acq_set_refine(nref)
        if any(getattr(c, "cdop", False) for c in channels):
            self.acq_set_codedoppler([c.f_cf if getattr(c, "cdop", False) else 0.0 for c in channels])

    # -- tracking
    def trk_set_state(self, states, ch0=0):
        arr = (TrkState * len(states))()
        for i, s in enumerate(states):
            arr[i].carrfreq, arr[i].codefreq = s["carrfreq"], s["codefreq"]
            arr[i].remcode, arr[i].remcarr, arr[i].buffloc = s["remcode"], s["remcarr"], s["buffloc"]
        _check(self._L.gnsscorr_trk_set_state(self.h, ch0, len(states), arr))

    def trk_get_state(self, ch0=0, nch=None):
        nch = len(self.channels) - ch0 if nch is None else nch
        arr = (TrkState * nch)()
        _check(self._L.gnsscorr_trk_get_state(self.h, ch0, nch, arr))
        return [dict(carrfreq=a.carrfreq, codefreq=a.codefreq, remcode=a.remcode, remcarr=a.remcarr,
                     buffloc=a.buffloc) for a in arr]

    def trk_run(self, nepoch):
        _check(self._L.gnsscorr_trk_run(self.h, nepoch))
        self._nepoch = nepoch

    def trk_fetch(self):
        nch, ne, nt = len(self.channels), self._nepoch, self.channels[0].ntap
        II = np.empty((nch, ne, nt), np.float64)
        QQ = np.empty((nch, ne, nt), np.float64)
        ns = np.empty((nch, ne), np.int32)
        _check(self._L.gnsscorr_trk_fetch(self.h, II.ctypes.data, QQ.ctypes.data, ns.ctypes.data))
        return II, QQ, ns

    def trk_fetch_sums(self):
        nch, nt = len(self.channels), self.channels[0].ntap
        sI = np.empty((nch, nt), np.float64)
        sQ = np.empty((nch, nt), np.float64)
        _check(self._L.gnsscorr_trk_fetch_sums(self.h, sI.ctypes.data, sQ.ctypes.data))
        return sI, sQ

    def trk_devptrs(self):
        """(II, QQ) device addresses of the last run's result arrays as integers, laid out as trk_fetch returns them
        (gnsscorr_trk_devptrs): work queued on the context's stream after this call sees every trk_run issued before
        it.  The addresses change when a longer batch makes the arrays grow."""
        II, QQ = C.c_void_p(), C.c_void_p()
        _check(self._L.gnsscorr_trk_devptrs(self.h, C.byref(II), C.byref(QQ)))
        return int(II.value or 0), int(QQ.value or 0)

    # -- closed loop
    def loop_state(self, ch, acqfreq, dllb=(5.0, 1.0), pllb=(30.0, 10.0), fllb=(200.0, 50.0), flagsync=0, synci=0,
                   cnt=0, loop=None):
        """A LoopState for channel index `ch` with the constants inittrkprmstruct()/inittrkstruct() derive
        (ref src/sdrinit.c:402-425,432-480) and zeroed filter state."""
        c = self.channels[ch]
        ls = LoopState()
        ls.acqfreq, ls.f_if, ls.foffset, ls.f_cf, ls.crate, ls.ctime = acqfreq, c.f_if, c.foffset, c.f_cf, c.crate, c.ctime
        for i in range(2):
            ls.dllw2[i] = (dllb[i] / 0.53) * (dllb[i] / 0.53)
            ls.dllaw[i] = 1.414 * (dllb[i] / 0.53)
            ls.pllw2[i] = (pllb[i] / 0.53) * (pllb[i] / 0.53)
            ls.pllaw[i] = 1.414 * (pllb[i] / 0.53)
            ls.fllw[i] = fllb[i] / 0.25
        ls.ne, ls.nl = c.ne, c.nl
        loop = loop if loop is not None else (2 if c.ctype == CTYPE_L1SBAS else 10)
        ls.loopms = loop * int(c.ctime * 1000)
        ls.rate = 10 if c.ctype == CTYPE_G1 else (2 if c.ctype == CTYPE_L1SBAS else 20)
        ls.flagsync, ls.synci, ls.cnt = flagsync, synci, cnt
        ls.prn = c.prn
        return ls

    def loop_set(self, states, ch0=0):
        arr = (LoopState * len(states))(*states)
        _check(self._L.gnsscorr_loop_set(self.h, ch0, len(states), arr))

    def loop_get(self, ch0=0, nch=None):
        nch = len(self.channels) - ch0 if nch is None else nch
        arr = (LoopState * nch)()
        _check(self._L.gnsscorr_loop_get(self.h, ch0, nch, arr))
        return list(arr)

    def trk_run_loop(self, nperiod):
        _check(self._L.gnsscorr_trk_run_loop(self.h, nperiod))
        self._nepoch = nperiod

    def trk_fetch_log(self):
        nch = len(self.channels)
        log = np.zeros((nch, self._nepoch), dtype=np.dtype(TrkLog))
        ndone = np.zeros(nch, np.int32)
        _check(self._L.gnsscorr_trk_fetch_log(self.h, log.ctypes.data, ndone.ctypes.data))
        return log, ndone

    def trk_loop_lapped(self):
        """Periods of the last trk_run_loop that read samples the writer had overwritten since."""
        n = C.c_int()
        _check(self._L.gnsscorr_trk_loop_lapped(self.h, C.byref(n)))
        return n.value

    # -- acquisition
    def acq_run(self, wrpos=0, channels=None):
        """channels: None searches every channel (gnsscorr_acq_run), a sequence of distinct channel indices only
        those (gnsscorr_acq_run_subset)."""
        if channels is None:
            _check(self._L.gnsscorr_acq_run(self.h, wrpos))
        else:
            arr = (C.c_int * len(channels))(*channels)
            _check(self._L.gnsscorr_acq_run_subset(self.h, wrpos, arr, len(channels)))

    def acq_set_coherent(self, ncoh, ch0=0):
        """Code periods channels ch0 .. ch0+len(ncoh)-1 integrate coherently per group (gnsscorr_acq_set_coherent);
        set_channels resets every channel to 1 and then applies the channels' own ncoh."""
        arr = (C.c_int * len(ncoh))(*ncoh)
        _check(self._L.gnsscorr_acq_set_coherent(self.h, ch0, len(ncoh), arr))

    def acq_get_coherent(self, ch0=0, nch=None):
        nch = len(self.channels) - ch0 if nch is None else nch
        arr = (C.c_int * nch)()
        _check(self._L.gnsscorr_acq_get_coherent(self.h, ch0, nch, arr))
        return list(arr)

    def acq_set_bitedge(self, estep, ch0=0):
        """Bit-edge step of channels ch0 .. ch0+len(estep)-1 (gnsscorr_acq_set_bitedge: hypotheses h = 0, estep, ... <
        ncoh per coherent group, 0: none).  set_channels and acq_set_coherent reset it to 0; set_channels then applies
        the channels' own ncoh and estep, in that order."""
        arr = (C.c_int * len(estep))(*estep)
        _check(self._L.gnsscorr_acq_set_bitedge(self.h, ch0, len(estep), arr))

    def acq_get_bitedge(self, ch0=0, nch=None):
        nch = len(self.channels) - ch0 if nch is None else nch
        arr = (C.c_int * nch)()
        _check(self._L.gnsscorr_acq_get_bitedge(self.h, ch0, nch, arr))
        return list(arr)

    def acq_fetch_edge(self):
        """Per channel the bit edge the last search decided on (gnsscorr_acq_fetch_edge): the hypothesis h* of the
        deciding group's best row, 0 for no edge; -1 for a channel that was not listed, not acquired or has estep 0."""
        arr = (C.c_int * len(self.channels))()
        _check(self._L.gnsscorr_acq_fetch_edge(self.h, arr))
        return list(arr)

    def acq_set_codedoppler(self, f_cf, ch0=0):
        """RF carrier (Hz) channels ch0 .. ch0+len(f_cf)-1 compensate code Doppler with across the groups of a search
        (gnsscorr_acq_set_codedoppler; 0: off, what set_channels resets to before it applies Channel.cdop)."""
        arr = (C.c_double * len(f_cf))(*[float(v) for v in f_cf])
        _check(self._L.gnsscorr_acq_set_codedoppler(self.h, ch0, len(f_cf), arr))

    def acq_get_codedoppler(self, ch0=0, nch=None):
        nch = len(self.channels) - ch0 if nch is None else nch
        arr = (C.c_double * nch)()
        _check(self._L.gnsscorr_acq_get_codedoppler(self.h, ch0, nch, arr))
        return list(arr)

    def acq_fetch_shifts(self, ch):
        """(s, back) of channel ch as the last prepare built them (gnsscorr_acq_fetch_shifts): s an int32 array
        [nfreq][groups], back the samples the search looks back beyond (intg + 1) * nsamp."""
        c = self.channels[ch]
        ncoh = self.acq_get_coherent(ch, 1)[0]
        s = np.zeros((c.nfreq, c.intg // ncoh), np.int32)
        back = C.c_int(0)
        _check(self._L.gnsscorr_acq_fetch_shifts(self.h, ch, s.ctypes.data, C.byref(back)))
        return s, back.value

    def acq_set_refine(self, nref, ch0=0):
        """Code periods channels ch0 .. ch0+len(nref)-1 refine their carrier frequency over after a search acquires
        them (gnsscorr_acq_set_refine: 0 off, else 2 .. min(intg, MAXCOH)); set_channels resets every channel to 0 and
        then applies the channels' own nref."""
        arr = (C.c_int * len(nref))(*nref)
        _check(self._L.gnsscorr_acq_set_refine(self.h, ch0, len(nref), arr))

    def acq_get_refine(self, ch0=0, nch=None):
        nch = len(self.channels) - ch0 if nch is None else nch
        arr = (C.c_int * nch)()
        _check(self._L.gnsscorr_acq_get_refine(self.h, ch0, nch, arr))
        return list(arr)

    def acq_fetch_fine(self, prompts=False):
        """Per channel the refinement of the last search (gnsscorr_acq_fetch_fine): dicts of finefreq, quality, q and
        nref (nref 0: none, finefreq is the bin centre).  prompts=True: also the prompt sums, int32 [nch][MAXCOH][2]
        (I, Q of P_m, zero beyond nref)."""
        nch = len(self.channels)
        arr = (AcqFine * nch)()
        P = np.zeros((nch, MAXCOH, 2), np.int32) if prompts else None
        _check(self._L.gnsscorr_acq_fetch_fine(self.h, arr, P.ctypes.data if prompts else None))
        fine = [dict(finefreq=a.finefreq, quality=a.quality, q=a.q, nref=a.nref) for a in arr]
        return (fine, P) if prompts else fine

    def acq_fetch(self):
        arr = (AcqRes * len(self.channels))()
        _check(self._L.gnsscorr_acq_fetch(self.h, arr))
        return [dict(acqcodei=a.acqcodei, freqi=a.freqi, acqfreq=a.acqfreq, cn0=a.cn0, peakr=a.peakr,
                     flagacq=a.flagacq, iters=a.iters, buffloc=a.buffloc) for a in arr]

    def trk_start_from_acq(self):
        _check(self._L.gnsscorr_trk_start_from_acq(self.h))

    def loop_start_from_acq(self):
        """Device hand-over of the last search's acquired channels into the closed loop (tracking and loop state)."""
        _check(self._L.gnsscorr_loop_start_from_acq(self.h))

    def acq_power(self, ch):
        c = self.channels[ch]
        P = np.empty((c.nfreq, c.nsamp), np.float64)
        _check(self._L.gnsscorr_acq_power(self.h, ch, P.ctypes.data))
        return P

    # -- receiver schedule
    def rx_start(self, retry_ms=0):
        """Every channel -> SEARCH (gnsscorr_rx_start); retry_ms <= 0: ACQSLEEP."""
        _check(self._L.gnsscorr_rx_start(self.h, int(retry_ms)))

    def rx_set(self, ch, state):
        _check(self._L.gnsscorr_rx_set(self.h, ch, state))

    def rx_step(self, max_periods):
        """One scheduling step at the rings' current write positions; its tracking part reports through trk_fetch /
        trk_fetch_log like trk_run_loop(max_periods)."""
        _check(self._L.gnsscorr_rx_step(self.h, max_periods))
        self._nepoch = max_periods

    def rx_status(self):
        arr = (RxStat * len(self.channels))()
        _check(self._L.gnsscorr_rx_status(self.h, arr))
        return [dict(state=a.state, attempts=a.attempts, next_try=a.next_try, acq_wrpos=a.acq_wrpos, cnt=a.cnt,
                     acq=dict(acqcodei=a.acq.acqcodei, freqi=a.acq.freqi, acqfreq=a.acq.acqfreq, cn0=a.acq.cn0,
                              peakr=a.acq.peakr, flagacq=a.acq.flagacq, iters=a.acq.iters, buffloc=a.acq.buffloc))
                for a in arr]

    # -- frames, observables and epochs behind every step
    def rx_nav_start(self, outms, hold_steps=0):
        """Switches the nav driver on (gnsscorr_rx_nav_start): with the schedule, before its first step."""
        _check(self._L.gnsscorr_rx_nav_start(self.h, int(outms), int(hold_steps)))

    def rx_nav_step(self, max_periods):
        """rx_step (schedule on) or trk_run_loop (off) of max_periods, and the feed of its rows; the plain fetches stay
        valid behind it."""
        _check(self._L.gnsscorr_rx_nav_step(self.h, int(max_periods)))
        self._nepoch = max_periods

    def rx_nav(self):
        """The context's RxNav (week, fetch, flush, status, frame, rows), or None while the driver is off.  The context
        owns it: the wrapper is good until the driver is switched off."""
        h = self._L.gnsscorr_rx_nav(self.h)
        return RxNav(handle=h) if h else None

    def rx_nav_stop(self):
        _check(self._L.gnsscorr_rx_nav_stop(self.h))

    def trk_fetch_prompt(self):
        """(II0, QQ0) [nch][nperiod]: tap 0 of trk_fetch's II and QQ, gathered on the device."""
        nch, ne = len(self.channels), self._nepoch
        II0 = np.empty((nch, ne), np.float64)
        QQ0 = np.empty((nch, ne), np.float64)
        _check(self._L.gnsscorr_trk_fetch_prompt(self.h, II0.ctypes.data, QQ0.ctypes.data))
        return II0, QQ0

    # -- the schedule's stages: what the three rx_*_set and the three *_run wrappers share
    def _rx_stage_set(self, fn, make, prm, ch0, nch):
        nch = len(self.channels) - ch0 if nch is None else nch
        if isinstance(prm, dict):
            prm = make(**prm)
        _check(fn(self.h, ch0, nch, C.byref(prm) if prm is not None else None))

    @staticmethod
    def _stage_arrays(who, prm_t, st_t, prm, rate, st, I, Q, log, ndone, cnt0, taps=()):
        """The *_run arguments as the library reads them, I / Q [nch][nper] + taps; shapes and st checked."""
        I = np.ascontiguousarray(I, dtype=np.float64)
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        nch, nper = I.shape[:2]
        prm = np.ascontiguousarray(prm, dtype=np.dtype(prm_t))
        rate = np.ascontiguousarray(rate, dtype=np.int32)
        log = np.ascontiguousarray(log, dtype=np.dtype(TrkLog))
        ndone = np.ascontiguousarray(ndone, dtype=np.int32)
        cnt0 = np.ascontiguousarray(cnt0, dtype=np.uint64)
        if not (Q.shape == I.shape == (nch, nper) + taps and log.shape == (nch, nper) and
                prm.shape == rate.shape == ndone.shape == cnt0.shape == st.shape == (nch,)):
            raise ValueError("%s: array shapes" % who)
        if st.dtype != np.dtype(st_t) or not st.flags.c_contiguous:
            raise ValueError("%s: st must be a contiguous array of %s" % (who, st_t.__name__))
        return prm, rate, I, Q, log, ndone, cnt0, nch, nper

    # -- lock monitor
    def rx_lock_set(self, prm=None, ch0=0, nch=None):
        """The lock monitor's parameters for channels ch0 .. ch0+nch-1 (default: all from ch0 on): a LockPrm, a dict of
        its fields, or None to switch it off."""
        self._rx_stage_set(self._L.gnsscorr_rx_lock_set, LockPrm, prm, ch0, nch)

    def rx_lock_status(self):
        """(states, losses): numpy arrays [nch] of LockState and of int32 (gnsscorr_rx_lock_status)."""
        nch = len(self.channels)
        st = np.zeros(nch, dtype=np.dtype(LockState))
        losses = np.zeros(nch, np.int32)
        _check(self._L.gnsscorr_rx_lock_status(self.h, st.ctypes.data, losses.ctypes.data))
        return st, losses

    def lock_run(self, prm, rate, st, I, Q, log, ndone, cnt0):
        """gnsscorr_lock_run: prm [nch] of LockPrm, rate [nch], st [nch] of LockState (updated in place), I / Q
        [nch][nper], log [nch][nper] of TrkLog, ndone [nch], cnt0 [nch].  Returns st."""
        prm, rate, I, Q, log, ndone, cnt0, nch, nper = self._stage_arrays("lock_run", LockPrm, LockState, prm, rate, st, I, Q, log, ndone, cnt0)
        _check(self._L.gnsscorr_lock_run(self.h, prm.ctypes.data, rate.ctypes.data, st.ctypes.data, I.ctypes.data, Q.ctypes.data,
               log.ctypes.data, ndone.ctypes.data, cnt0.ctypes.data, nch, nper))
        return st

    # -- bit synchronisation by symbol energy
    def rx_bsync_set(self, prm=None, ch0=0, nch=None):
        """The bit-synchronisation detector's parameters for channels ch0 .. ch0+nch-1 (default: all from ch0 on): a
        BsyncPrm, a dict of its fields, or None to switch it off."""
        self._rx_stage_set(self._L.gnsscorr_rx_bsync_set, BsyncPrm, prm, ch0, nch)

    def rx_bsync_status(self):
        """(states, applied): numpy arrays [nch] of BsyncState and of int32 (gnsscorr_rx_bsync_status)."""
        nch = len(self.channels)
        st = np.zeros(nch, dtype=np.dtype(BsyncState))
        applied = np.zeros(nch, np.int32)
        _check(self._L.gnsscorr_rx_bsync_status(self.h, st.ctypes.data, applied.ctypes.data))
        return st, applied

    def bsync_run(self, prm, rate, st, I, Q, log, ndone, cnt0):
        """gnsscorr_bsync_run: prm [nch] of BsyncPrm, rate [nch], st [nch] of BsyncState (updated in place), I / Q
        [nch][nper], log [nch][nper] of TrkLog, ndone [nch], cnt0 [nch].  Returns st."""
        prm, rate, I, Q, log, ndone, cnt0, nch, nper = self._stage_arrays("bsync_run", BsyncPrm, BsyncState, prm, rate, st, I, Q, log, ndone, cnt0)
        _check(self._L.gnsscorr_bsync_run(self.h, prm.ctypes.data, rate.ctypes.data, st.ctypes.data, I.ctypes.data, Q.ctypes.data,
               log.ctypes.data, ndone.ctypes.data, cnt0.ctypes.data, nch, nper))
        return st

    # -- correlation monitor
    def rx_cfm_set(self, prm=None, ch0=0, nch=None):
        """The correlation monitor's parameters for channels ch0 .. ch0+nch-1 (default: all from ch0 on): a CfmPrm, a
        dict of its fields (dref / rref: sequences of up to 16 values, the rest 0), or None to switch it off."""
        self._rx_stage_set(self._L.gnsscorr_rx_cfm_set, cfm_prm, prm, ch0, nch)

    def rx_cfm_status(self):
        """numpy array [nch] of CfmState (gnsscorr_rx_cfm_status)."""
        st = np.zeros(len(self.channels), dtype=np.dtype(CfmState))
        _check(self._L.gnsscorr_rx_cfm_status(self.h, st.ctypes.data))
        return st

    def cfm_run(self, prm, rate, corrn, st, II, QQ, log, ndone, cnt0):
        """gnsscorr_cfm_run: prm [nch] of CfmPrm, rate [nch], corrn, st [nch] of CfmState (updated in place), II / QQ
        [nch][nper][1+2*corrn], log [nch][nper] of TrkLog, ndone [nch], cnt0 [nch].  Returns st."""
        prm, rate, II, QQ, log, ndone, cnt0, nch, nper = self._stage_arrays("cfm_run", CfmPrm, CfmState, prm, rate, st, II, QQ, log, ndone, cnt0,
                                                                             (1 + 2 * corrn,))
        _check(self._L.gnsscorr_cfm_run(self.h, prm.ctypes.data, rate.ctypes.data, corrn, st.ctypes.data, II.ctypes.data,
               QQ.ctypes.data, log.ctypes.data, ndone.ctypes.data, cnt0.ctypes.data, nch, nper))
        return st

    # -- IF monitor
    def spectrum(self, ftype, buffloc, n, f_sf, nfft=16384, nloop=SPEC_NLOOP, offsets=None, seed=None):
        """Sample histogram and Hann-windowed averaged power spectrum of ring `ftype` (gnsscorr_spec_run/fetch):
        what specthread() gets from calchistgram() + spectrumanalyzer() (ref src/sdrspec.c:64-102).
        buffloc: first sample of a snapshot, or a sequence of them.  offsets: [nsnap][nloop] segment starts in
        [0, n - nfft/2]; None draws them with numpy.random.default_rng(seed).
        Returns (freq [dtype*nfft] MHz, pspec dB [nsnap][dtype*nfft], s linear [nsnap][2*nfft],
        hist [nsnap][2][9]); the nsnap axis is dropped for an int buffloc."""
        single = np.ndim(buffloc) == 0
        loc = np.ascontiguousarray(np.atleast_1d(buffloc), dtype=np.uint64)
        nsnap = loc.size
        if offsets is None:
            offsets = np.random.default_rng(seed).integers(0, n - nfft // 2 + 1, size=(nsnap, nloop))
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(nsnap, nloop)
        sp = SpecParams(ftype, nfft, nloop, n, float(f_sf))
        _check(self._L.gnsscorr_spec_run(self.h, C.byref(sp), nsnap, loc.ctypes.data, off.ctypes.data))
        dtype = self._ring_dtype[ftype]
        s = np.empty((nsnap, 2 * nfft))
        pspec = np.empty((nsnap, dtype * nfft))
        freq = np.empty(dtype * nfft)
        hist = np.empty((nsnap, 2, SPEC_HIST), np.int64)
        _check(self._L.gnsscorr_spec_fetch(self.h, s.ctypes.data, s.size, pspec.ctypes.data, pspec.size,
                                           freq.ctypes.data, freq.size, hist.ctypes.data, hist.size))
        if single:
            return freq, pspec[0], s[0], hist[0]
        return freq, pspec, s, hist

    # -- FEC / SBAS frame synchronisation
    def fec_run(self, sym, pos0, npos, stride=1, win=1512, ndec=750, polyA=V27POLYA, polyB=V27POLYB, rowbytes=None):
        """gnsscorr_fec_run on sym[nch][nsym] (or [nsym]) of +-1 / 0: uint8 rows [nch][npos][rowbytes], the ndec decoded
        bits of the window that ends at symbol pos0 + p*stride packed MSB first (np.unpackbits gives them back)."""
        a = np.ascontiguousarray(np.atleast_2d(sym), dtype=np.int8)
        nch, nsym = a.shape
        rowbytes = (ndec + 7) // 8 if rowbytes is None else rowbytes
        out = np.zeros((nch, max(npos, 0), max(rowbytes, 0)), np.uint8)
        buf = out if out.size else np.zeros(1, np.uint8)
        _check(self._L.gnsscorr_fec_run(self.h, a.ctypes.data, nch, nsym, pos0, npos, stride, win, ndec, polyA, polyB,
                                        buf.ctypes.data, rowbytes))
        return out

    def sbasframe_replay(self, state, log_rows, cnt0=0, aid_tow=None, aid_week=0):
        """The symbols of one channel's log rows (numpy array of TrkLog) through the SBAS frame synchronisation: Viterbi
        decodes on this engine's device, the walk on the host; `state` (SbasFrameState) is updated."""
        log_rows = np.ascontiguousarray(log_rows)
        n = int(log_rows.shape[0])
        aid = None
        if aid_tow is not None:
            aid = np.ascontiguousarray(aid_tow, dtype=np.float64)
            if aid.shape != (n,):
                raise ValueError("aid_tow: one value per log row")
        rc = self._L.gnsscorr_sbasframe_replay(self.h, C.byref(state), log_rows.ctypes.data, n, int(cnt0),
                                               aid.ctypes.data if aid is not None else None, int(aid_week))
        if rc:
            raise GnsscorrError("gnsscorr_sbasframe_replay: error %d (%s)" % (rc, lib().gnsscorr_last_error().decode()))

    def debug_fec_parts(self, parts):
        """(tools) 3: the decoder; 1 / 2: the forward pass / the chainback of fec_viterbi27 alone (rows are no decodes)."""
        _check(self._L.gnsscorr_debug_fec_parts(self.h, parts))

    # -- timing
    def timing(self, on=True):
        _check(self._L.gnsscorr_timing_enable(self.h, int(on)))

    def timing_reset(self):
        _check(self._L.gnsscorr_timing_reset(self.h))

    def timing_read(self, kernel):
        ms, n = C.c_double(), C.c_int()
        _check(self._L.gnsscorr_timing_read(self.h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value
