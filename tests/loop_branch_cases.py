"""Case tables for the closed loop's filter branches, the vote path of checksync() and the filter cadences
(tests/test_loop_branch_host.py on the CPU, tests/test_gpu_loop_branches.py on the device).

No signal is synthesised.  gnsscorr_loop_t and the oracle's Chan carry the same fields, so a case is a set of presets,
applied to both by `apply_presets`:

* filter rows run on a ring of zeros: the period's correlator adds exactly 0.0 to the preset sums, and with
  flagsync = 0 the prm1 filters run on exactly those values (a preset of -0.0 becomes +0.0 there: -0.0 + 0.0 = +0.0 in
  round-to-nearest; only a direct call of the filters sees a -0.0 sum);
* nav and cadence rows run on seeded int8 noise: the vote histogram is preset one vote short of the threshold, so the
  first sign change of the prompt at the preset position synchronises the channel.

Every row names the branch it is made for and carries what the oracle alone has to show for it (`expect`);
test_loop_branch_host.py asserts that, row by row.  restate_pll / restate_dll restate the two filters
(ref src/sdrtrk.c:95-150) in mpmath at 50 digits, the special cases from IEEE 754 / C Annex F."""
import math

import mpmath
import numpy as np

mp = mpmath.mp.clone()
mp.dps = 50
PI_D = 3.1415926535897932           # the reference's PI (ref src/sdr.h:103), a double
NAN = float("nan")

# ---- presets ------------------------------------------------------------------------------------------------------
ARRAY_FIELDS = ("II", "QQ", "oldI", "oldQ", "sumI", "sumQ", "oldsumI", "oldsumQ", "bitsync")


def apply_presets(obj, presets):
    """The same presets on a LoopState or an oracle Chan.  Array fields (sums, bitsync) take {index: value}."""
    for name, v in presets.items():
        if name in ARRAY_FIELDS:
            arr = getattr(obj, name)
            for i, x in v.items():
                arr[i] = x
        else:
            setattr(obj, name, v)


def make_ring_data(kind, dtype, nsamples, seed=7):
    """The IF samples of a case: 'zero', or int8 noise in -60..60 from `seed` (IQ pairs for dtype 2)."""
    shape = (nsamples, 2) if dtype == 2 else (nsamples,)
    if kind == "zero":
        return np.zeros(shape, np.int8)
    return np.random.default_rng(seed).integers(-60, 61, size=shape, dtype=np.int8)


def start_state(i, f_if, crate, nsamp, seed):
    """Channel i's NCO state at the start of a noise case: anywhere in +-5 kHz, remainders and ring position random."""
    rng = np.random.default_rng([seed, i])
    return dict(carrfreq=f_if + float(rng.uniform(-5000, 5000)), codefreq=crate + float(rng.uniform(-3, 3)),
                remcode=float(rng.uniform(0.01, 0.99)), remcarr=float(rng.uniform(0, 6.2)),
                buffloc=int(rng.integers(0, nsamp)))


def acqfreq_of(st, f_if):
    return f_if + 200.0 * round((st["carrfreq"] - f_if) / 200.0)       # the 200 Hz grid of sdracquisition()


def oracle_chan(orc, row, st, dtype, f_sf, f_if, taps):
    """The oracle's channel for `row` from NCO state `st`."""
    corrn, corrd, corrp = taps
    o = orc.make_chan(row["prn"], dtype=dtype, f_sf=f_sf, f_if=f_if, corrn=corrn, corrd=corrd, corrp=corrp)
    o.acq.acqfreq = acqfreq_of(st, f_if)
    o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
    apply_presets(o, row["presets"])
    return o


# ---- the filter table -----------------------------------------------------------------------------------------------
# Presets of the filters' own state, so that the difference terms (carrErr - old carrErr, ...) count
FILTER_STATE = dict(carrErr=0.0125, codeErr=-0.03, carrNco=3.75, codeNco=-0.4)
# E/L sums of the PLL rows and prompt sums of the DLL rows (an ordinary case of the other filter)
_EL = dict(IE=300.0, QE=-400.0, IL=250.0, QL=120.0)
_P = dict(IP=3000.0, QP=450.0, oldIP=2900.0, oldQP=-380.0)


def _frow(name, branch, **kw):
    sums = dict(_P, **_EL)
    sums.update(kw)
    return dict(name=name, branch=branch, sums=sums)


# branch: what the host test asserts the row reaches -- (sign class of IP, f1 special, f2 special, wrap) for the PLL,
# the DLL's case for the DLL rows.  wrap: +1 / -1 the upper / lower wrap fired, 0 none.
FILTER_ROWS = [
    _frow("pll_ip_pos", dict(ip="pos", wrap=0), IP=3000.0, QP=450.0, oldIP=2900.0, oldQP=-380.0),
    _frow("pll_ip_neg", dict(ip="neg", wrap=0), IP=-3000.0, QP=450.0, oldIP=-2900.0, oldQP=-380.0),
    _frow("pll_ip_zero_qp_pos", dict(ip="+0", wrap=0, carrErr=-0.5), IP=0.0, QP=400.0, oldIP=2900.0, oldQP=2000.0),
    _frow("pll_ip_zero_qp_neg", dict(ip="+0", wrap=0, carrErr=0.5), IP=0.0, QP=-400.0, oldIP=2900.0, oldQP=2000.0),
    _frow("pll_all_zero", dict(ip="+0", wrap=0, carrErr=-1.0, freqErr=0.0), IP=0.0, QP=0.0, oldIP=0.0, oldQP=0.0),
    _frow("pll_ip_negzero_qp_pos", dict(ip="-0", wrap=0), IP=-0.0, QP=400.0, oldIP=2900.0, oldQP=2000.0),
    _frow("pll_ip_negzero_qp_zero", dict(ip="-0", wrap=0), IP=-0.0, QP=0.0, oldIP=2900.0, oldQP=2000.0),
    _frow("pll_oldip_zero", dict(ip="pos", oldip0=True, wrap=0), IP=3000.0, QP=450.0, oldIP=0.0, oldQP=777.0),
    _frow("pll_wrap_far_over", dict(ip="pos", wrap=+1), IP=5.0, QP=4000.0, oldIP=-5.0, oldQP=4000.0),
    _frow("pll_wrap_just_over", dict(ip="pos", wrap=+1), IP=1.0, QP=1000.0, oldIP=1000.0, oldQP=-3.0),
    _frow("pll_nowrap_just_under", dict(ip="pos", wrap=0), IP=1.0, QP=1000.0, oldIP=1000.0, oldQP=1.0),
    _frow("pll_wrap_just_under_neg", dict(ip="neg", wrap=-1), IP=-1.0, QP=1000.0, oldIP=1000.0, oldQP=3.0),
    _frow("pll_nowrap_just_over_neg", dict(ip="neg", wrap=0), IP=-1.0, QP=1000.0, oldIP=1000.0, oldQP=-1.0),
    _frow("pll_freqerr_exactly_half_pi", dict(ip="+0", wrap=0, freqErr=PI_D / 2), IP=0.0, QP=400.0, oldIP=2900.0, oldQP=0.0),
    _frow("dll_e_gt_l", dict(dll="E>L"), IE=300.0, QE=-400.0, IL=250.0, QL=120.0),
    _frow("dll_e_lt_l", dict(dll="E<L"), IE=30.0, QE=-40.0, IL=250.0, QL=120.0),
    _frow("dll_e_eq_l", dict(dll="E=L", codeErr=0.0), IE=300.0, QE=-400.0, IL=-400.0, QL=300.0),
    _frow("dll_e_zero", dict(dll="E=0", codeErr=-1.0), IE=0.0, QE=0.0, IL=250.0, QL=120.0),
    _frow("dll_l_zero", dict(dll="L=0", codeErr=1.0), IE=300.0, QE=-400.0, IL=0.0, QL=0.0),
    _frow("dll_both_zero", dict(dll="0/0", codeErr=NAN), IE=0.0, QE=0.0, IL=0.0, QL=0.0),
]
# Rows whose preset IP is -0.0 reach the filters as -0.0 only in a direct call; through a period's cumsumcorr they are
# +0.0 and give the +0.0 rows' values:
NEGZERO_AS_STEP = {"pll_ip_negzero_qp_pos": dict(carrErr=-0.5), "pll_ip_negzero_qp_zero": dict(carrErr=-1.0)}


def filter_presets(row, ne, nl):
    """gnsscorr_loop_t / Chan presets of a filter row for early / late tap indices ne / nl: every II/QQ/oldI/oldQ tap 0
    (as both sides initialise them), the sums at taps 0, ne, nl."""
    s = row["sums"]
    p = dict(FILTER_STATE)
    p.update(flagsync=0, cnt=0,
             sumI={0: s["IP"], ne: s["IE"], nl: s["IL"]}, sumQ={0: s["QP"], ne: s["QE"], nl: s["QL"]},
             oldsumI={0: s["oldIP"]}, oldsumQ={0: s["oldQP"]})
    return p


FILTER_F_SF = 16.368e6


def filter_start(i, f_if, crate):
    """NCO state of filter row i's channel at the start of its one period."""
    return dict(carrfreq=f_if + 1433.25 + 10.0 * i, codefreq=crate + 0.3, remcode=0.3, remcarr=1.7, buffloc=100 + 7 * i)


def filter_oracle_chan(orc, row, i=0, taps=(2, 3, 3), dtype=2, f_if=0.0):
    """The oracle's channel for filter row `row` as channel i of its engine (PRN 6 + i: the vote path stays out)."""
    o = orc.make_chan(6 + i, dtype=dtype, f_sf=FILTER_F_SF, f_if=f_if, corrn=taps[0], corrd=taps[1], corrp=taps[2])
    st = filter_start(i, f_if, o.crate)
    o.acq.acqfreq = f_if + 1400.0
    o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
    apply_presets(o, filter_presets(row, o.ne, o.nl))
    return o


def restate_row(row, o, prm, dt, through_step):
    """The restatement on a row's sums with the constants of the oracle channel `o` (read before the filters run).
    through_step: the sums as a period's cumsumcorr leaves them (preset + 0.0).  -> (pll dict, carrfreq -> dll dict)."""
    s = {k: (v + 0.0 if through_step else v) for k, v in row["sums"].items()}
    st = FILTER_STATE
    p = restate_pll(s["IP"], s["QP"], s["oldIP"], s["oldQP"], st["carrErr"], st["carrNco"], o.pllaw[prm], o.pllw2[prm],
                    o.fllw[prm], dt, o.acq.acqfreq)
    return p, (lambda carrfreq: restate_dll(s["IE"], s["QE"], s["IL"], s["QL"], st["codeErr"], st["codeNco"], o.dllaw[prm],
                                            o.dllw2[prm], dt, o.crate, carrfreq, o.f_if, o.foffset, o.f_cf))


def exact_outputs(row, through_step):
    """The outputs of a row that are exact values (+-0.5, -1, 0, +-1, pi/2, NaN): {field: value}."""
    ex = {f: v for f, v in row["branch"].items() if f in ("carrErr", "freqErr", "codeErr")}
    if through_step and row["name"] in NEGZERO_AS_STEP:
        ex.update(NEGZERO_AS_STEP[row["name"]])
    return ex


# ---- restatement of the filters ---------------------------------------------------------------------------------------
def _is_negzero(x):
    return x == 0.0 and math.copysign(1.0, x) < 0


def _atan2(y, x):
    """atan2 of two doubles at 50 digits; zeros by C Annex F.10.1.4 (mpmath has no signed zero).  Returns an mpf, or
    the float -0.0 where the result is a negative zero."""
    if y == 0.0:
        neg = _is_negzero(y)
        if x < 0 or _is_negzero(x):
            return -mp.pi if neg else +mp.pi        # atan2(+-0, -0) = atan2(+-0, x < 0) = +-pi
        return -0.0 if neg else mp.mpf(0)           # atan2(+-0, +0) = atan2(+-0, x > 0) = +-0
    if x == 0.0:
        return -mp.pi / 2 if y < 0 else mp.pi / 2   # atan2(y, +-0) = +-pi/2
    return mp.atan2(mp.mpf(y), mp.mpf(x))


def _neg(x):
    return -x                                        # (on a float: -(+0.0) = -0.0)


def restate_pll(IP, QP, oldIP, oldQP, carrErr0, carrNco0, pllaw, pllw2, fllw, dt, acqfreq):
    """pll() (ref src/sdrtrk.c:95-126) on double inputs, every operation exact at 50 digits; PI is the reference's
    double constant.  -> dict(carrErr, freqErr, carrNco, carrfreq, f1mf2, wrap) of mpf (carrErr may be the float -0.0)."""
    PI = mp.mpf(PI_D)
    a = _atan2(QP, IP) if IP > 0 else _atan2(_neg(QP), _neg(IP))
    carrErr = a if isinstance(a, float) else a / PI
    f1 = PI / 2 if IP == 0 else mp.atan(mp.mpf(QP) / mp.mpf(IP))
    f2 = PI / 2 if oldIP == 0 else mp.atan(mp.mpf(oldQP) / mp.mpf(oldIP))
    d = f1 - f2
    freqErr, wrap = d, 0
    if freqErr > PI / 2:
        freqErr, wrap = PI - freqErr, +1
    if freqErr < -PI / 2:
        freqErr, wrap = -PI - freqErr, -1
    ce = mp.mpf(carrErr)
    carrNco = mp.mpf(carrNco0) + mp.mpf(pllaw) * (ce - mp.mpf(carrErr0)) + mp.mpf(pllw2) * mp.mpf(dt) * ce + \
        mp.mpf(fllw) * mp.mpf(dt) * freqErr
    return dict(carrErr=carrErr, freqErr=freqErr, carrNco=carrNco, carrfreq=mp.mpf(acqfreq) + carrNco, f1mf2=d, wrap=wrap)


def restate_dll(IE, QE, IL, QL, codeErr0, codeNco0, dllaw, dllw2, dt, crate, carrfreq, f_if, foffset, f_cf):
    """dll() (ref src/sdrtrk.c:135-150) likewise; carrfreq: the value pll() left (an mpf or a double).  0/0 is NaN
    (IEEE 754 7.2), and so is everything computed from it.  -> dict(codeErr, codeNco, codefreq)."""
    E = mp.sqrt(mp.mpf(IE) ** 2 + mp.mpf(QE) ** 2)
    L = mp.sqrt(mp.mpf(IL) ** 2 + mp.mpf(QL) ** 2)
    if E + L == 0:
        return dict(codeErr=NAN, codeNco=NAN, codefreq=NAN)
    codeErr = (E - L) / (E + L)
    codeNco = mp.mpf(codeNco0) + mp.mpf(dllaw) * (codeErr - mp.mpf(codeErr0)) + mp.mpf(dllw2) * mp.mpf(dt) * codeErr
    codefreq = mp.mpf(crate) - codeNco + (mp.mpf(carrfreq) - mp.mpf(f_if) - mp.mpf(foffset)) / (mp.mpf(f_cf) / mp.mpf(crate))
    return dict(codeErr=codeErr, codeNco=codeNco, codefreq=codefreq)


def ulps_from(value, restated):
    """Distance of the double `value` from the restated result, in ulps of that result rounded to double.  NaN where NaN
    is 0; NaN against a number, or a non-zero value against an exact 0, is inf."""
    if isinstance(restated, float) and math.isnan(restated):
        return 0.0 if math.isnan(value) else math.inf
    if math.isnan(value):
        return math.inf
    ref = float(restated)
    if ref == 0.0:
        return 0.0 if value == 0.0 else math.inf
    return float(abs(mp.mpf(value) - mp.mpf(restated)) / mp.mpf(math.ulp(ref)))


def same_double(a, b):
    """Bit for bit, NaN where NaN, -0.0 apart from +0.0."""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)


# ---- the nav and cadence tables ------------------------------------------------------------------------------------
# Front end of every noise case: int8 IQ at 4.092 Msps (4092 samples per code period), zero IF, 3 taps two samples apart
# (a one-sample offset leaves the reference's code remainder unwrapped: DESIGN.md section 3.1c)
NAV_FRONT = dict(dtype=2, f_sf=4.092e6, f_if=0.0, taps=(1, 2, 2))
NAV_NPER, NAV_CHUNKS, NAV_SEED = 130, (47, 83), 7
TWO32 = 1 << 32


def _nrow(name, prn, rate, loopms, cnt0, st, expect, bins=None, flagpol=0, flagsync=0, synci=0, navcnt=0):
    """st: index of the row's start state (start_state); rows that share it see the same prompt sums."""
    presets = dict(rate=rate, loopms=loopms, cnt=cnt0, flagpol=flagpol, flagsync=flagsync, synci=synci, navcnt=navcnt)
    if bins:
        presets["bitsync"] = {b: 50 for b in bins}
    return dict(name=name, prn=prn, st=st, presets=presets, expect=expect)


def _x(sync, synci, gaps, nupd, first, nbits):
    return dict(sync=sync, synci=synci, gaps=set(gaps), nupd=nupd, first=first, nbits=nbits)


# expect, found with the oracle alone and asserted by test_loop_branch_host.py before anything runs on a device:
#   sync   the period (0-based, of NAV_NPER) in which flagsync rises (0: preset), synci the bit edge it leaves;
#   gaps   the set of distances between filter updates (flagloopfilter == 2), nupd their number, first the first one's
#          period (None: none);  nbits  the number of decided bits.
# Vote rows (PRN <= 5): one bin of the histogram (two in one row) preset to NAVSYNCTH = 50 votes, every other bin 0;
# cnt0 > 2000, so checksync() runs from the first period; biti of period e is (cnt0 + e) % rate.
NAV_ROWS = [
    # bin 0 wins: synci-- goes below 0 and wraps to rate - 1; the next period has diffi = -rate + 1
    _nrow("vote_bin0_rate20_wrap", 1, 20, 10, 2001, 0, _x(19, 19, [10], 11, 28, 5), bins=[0]),
    _nrow("vote_bin7_rate20", 2, 20, 10, 2001, 1, _x(6, 6, [10], 12, 15, 6), bins=[7]),
    _nrow("vote_bin0_rate10_wrap", 3, 10, 10, 2001, 2, _x(9, 9, [10], 12, 18, 12), bins=[0]),
    # two bins one vote short: the prompt changes sign at position 12 (period 11) before it does at position 3
    _nrow("vote_two_bins_later_hit", 4, 20, 10, 2001, 3, _x(11, 11, [10], 11, 20, 5), bins=[3, 12]),
    # cnt crosses 2^32 before the vote falls: (2^32 - 40) % 20 = 16, and 2^32 % 20 = 16, not 0
    _nrow("vote_bin1_cnt_crosses_2_32", 5, 20, 10, TWO32 - 40, 6, _x(45, 0, [10], 8, 54, 4), bins=[1]),
    # the same start state with flagpol 1 and 0: the decided bits are each other's negatives
    _nrow("vote_bin0_rate2_flagpol1", 1, 2, 2, 2001, 7, _x(7, 1, [2], 61, 8, 61), bins=[0], flagpol=1),
    _nrow("vote_bin0_rate2_flagpol0", 1, 2, 2, 2001, 7, _x(7, 1, [2], 61, 8, 61), bins=[0], flagpol=0),
    _nrow("vote_bin7_rate20_flagpol1", 2, 20, 10, 2001, 9, _x(26, 6, [10], 10, 35, 5), bins=[7], flagpol=1),
    # loopms that does not divide rate, straight after a vote sync
    _nrow("vote_bin0_rate20_loopms3", 3, 20, 3, 2001, 10, _x(39, 19, [3, 5], 27, 41, 4), bins=[0]),
    _nrow("vote_bin0_rate10_loopms7", 5, 10, 7, 2001, 11, _x(19, 9, [10], 11, 25, 11), bins=[0]),
    # PRN > 5, rate 1: six prm1 periods (cnt 1995..2000), then the `rate == 1 && late` shortcut; biti - synci = 0 =
    # -rate + 1 in every period, so navcnt is 1 at every check: loopms 1 updates every period, loopms 2 never again
    _nrow("shift_rate1_loopms1", 12, 1, 1, 1995, 12, _x(6, 0, [1], 124, 6, 124)),
    _nrow("shift_rate1_loopms2", 13, 1, 2, 1995, 13, _x(6, 0, [], 0, None, 124)),
]
FLAGPOL_PAIR = ("vote_bin0_rate2_flagpol1", "vote_bin0_rate2_flagpol0")

# Cadence rows: flagsync = 1 preset, every loopms against every rate, synci and navcnt assorted.  (gaps, nupd, first, nbits)
CADENCE_LOOPMS, CADENCE_RATES = (1, 2, 3, 7, 10, 20, 25), (20, 10, 2, 1)
_CADENCE_EXPECT = {
    (1, 20): ([1], 130, 0, 7), (1, 10): ([1], 130, 0, 13), (1, 2): ([1], 130, 0, 65), (1, 1): ([1], 130, 0, 130),
    (2, 20): ([2, 3], 64, 1, 6), (2, 10): ([2], 65, 0, 13), (2, 2): ([2], 65, 0, 65), (2, 1): ([], 0, None, 130),
    (3, 20): ([3, 4, 5], 40, 1, 6), (3, 10): ([3, 4, 5], 39, 0, 13), (3, 2): ([], 0, None, 65), (3, 1): ([], 0, None, 130),
    (7, 20): ([7, 10, 13], 14, 0, 6), (7, 10): ([10], 12, 11, 13), (7, 2): ([], 0, None, 65), (7, 1): ([], 0, None, 130),
    (10, 20): ([10], 12, 16, 7), (10, 10): ([10], 12, 10, 13), (10, 2): ([], 1, 0, 65), (10, 1): ([], 0, None, 130),
    # a full 20-period interval; and the counter never reaches loopms (reset every `rate` periods): the interval is cut
    # at the step's capacity with no filter at its end -- one update where navcnt = 0 was preset, then none
    (20, 20): ([20], 6, 22, 7), (20, 10): ([], 1, 0, 13), (20, 2): ([], 0, None, 65), (20, 1): ([], 0, None, 130),
    (25, 20): ([], 1, 0, 6), (25, 10): ([], 0, None, 13), (25, 2): ([], 0, None, 65), (25, 1): ([], 0, None, 130),
}


def _cadence_rows():
    rows, i = [], 0
    for loopms in CADENCE_LOOPMS:
        for rate in CADENCE_RATES:
            g, nupd, first, nbits = _CADENCE_EXPECT[(loopms, rate)]
            synci = (3 + 7 * i) % rate
            rows.append(_nrow("cad_loopms%d_rate%d" % (loopms, rate), 1 + i, rate, loopms, 2001 + 3 * i, 100 + i,
                              _x(0, synci, g, nupd, first, nbits), flagsync=1, synci=synci, navcnt=i % 3))
            i += 1
    return rows


CADENCE_ROWS = _cadence_rows()
# cnt around 2^32 (nav_biti's 64-bit branch): a 32-bit remainder would move the bit phase by 16 * (cnt >> 32) mod 20
CNT_ROWS = [
    _nrow("cad_loopms3_rate20_cnt_crosses_2_32", 30, 20, 3, TWO32 - 40, 128, _x(0, 17, [3, 4, 5], 39, 0, 7),
          flagsync=1, synci=17, navcnt=0),
    _nrow("cad_loopms7_rate20_cnt_above_2_32", 31, 20, 7, 3 * TWO32 + 2001, 129, _x(0, 4, [7, 10, 13], 14, 5, 6),
          flagsync=1, synci=4, navcnt=2),
]
OBS_ROWS = ("cad_loopms3_rate20", "cad_loopms20_rate20")     # setobsdata replayed over the device's log for these


def run_oracle(orc, row, ring, nper=NAV_NPER, front=NAV_FRONT, seed=NAV_SEED):
    """`row` under the oracle alone, nper periods on `ring` (oracle.Ring of make_ring_data('noise', ...)).
    -> dict(sync, synci, gaps, nupd, first, nbits, bits, biti_at_sync, at_sync, cnt, finite, o)."""
    import ctypes as C
    o0 = orc.make_chan(row["prn"], dtype=front["dtype"], f_sf=front["f_sf"], f_if=front["f_if"], corrn=front["taps"][0],
                       corrd=front["taps"][1], corrp=front["taps"][2])
    st = start_state(row["st"], front["f_if"], o0.crate, o0.nsamp, seed)
    o = oracle_chan(orc, row, st, front["dtype"], front["f_sf"], front["f_if"], front["taps"])
    b = C.c_uint64(st["buffloc"])
    sync = 0 if o.flagsync else None
    synci, upd, bits, finite, biti_at_sync, at_sync = o.synci, [], [], True, None, None
    for e in range(nper):
        was = o.flagsync
        assert orc.lib().orc_sdrthread_step(C.byref(o), C.byref(ring), C.byref(b)) == 1, (row["name"], e)
        if o.flagsync and not was:
            sync, synci, biti_at_sync = e, o.synci, o.biti
            at_sync = (o.biti - o.synci, o.swreset)         # checkbit() of the same period: diffi and its reset
        if o.flagloopfilter == 2:
            upd.append(e)
        if o.flagsync and o.swsync:
            bits.append(o.bit)
        finite = finite and all(math.isfinite(getattr(o, f)) for f in ("carrfreq", "codefreq", "remcode", "remcarr")) \
            and o.currnsamp > 0
    gaps = set(int(x) for x in np.diff(upd))
    return dict(sync=sync, synci=synci, gaps=gaps, nupd=len(upd), first=upd[0] if upd else None, nbits=len(bits), bits=bits,
                biti_at_sync=biti_at_sync, at_sync=at_sync, cnt=o.cnt, finite=finite, o=o)
