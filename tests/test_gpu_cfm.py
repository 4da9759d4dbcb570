"""The correlation monitor's kernel through its op-level seam (-m gpu): gnsscorr_cfm_run against the restated rules
(tests/cfm_restate.py) on seeded synthetic rows, every field of gnsscorr_cfm_t compared as bytes.  The kernel gives a
channel a wavefront and four channels a workgroup, takes the rows in chunks of 64 and in groups of 8, and lane t owns
tap t: so five channels (a full workgroup and a partial one), 130 rows (two chunks and a partial one), 3, 5 and 33 taps,
rates 2, 10 and 20 side by side, and row counts of 0, 1, 64, 65 and all."""
import numpy as np
import pytest

import cfm_restate as cr

pytestmark = pytest.mark.gpu
NCH, NPER = 5, 130
RATES = [20, 10, 2, 2, 10]
NDONE = [NPER, 65, 64, 1, 0]
CNT0 = [0, (1 << 32) + 5, 1000, 7, 0]
CORRNS = [1, 2, 16]


@pytest.fixture(scope="module")
def eng(gc):
    e = gc.Engine(0)
    yield e
    e.close()


def _rows(rng, nper, rate, ntap, first_sync, extra_end=None):
    """Unsynchronised rows up to first_sync, then bits of `rate` rows of random sign whose last row carries the decided
    bit (now and then the wrong one); extra_end: a row that ends a bit early, so that a short bit and the rest of it
    are dropped.  Taps: a triangle around the prompt plus noise, multiples of 1/32 near 2^24 -- the squares and the
    window sums do not fit a double, so every rounding counts."""
    amp = 2.0 ** 24
    shape = np.array([1.0] + [max(0.0, 1.0 - 0.5 * ((t + 1) // 2)) for t in range(1, ntap)])
    II, QQ = np.zeros((nper, ntap)), np.zeros((nper, ntap))
    fs, nb = np.zeros(nper, np.int32), np.zeros(nper, np.int32)
    off = int(rng.integers(0, rate))
    sign = rng.choice([-1.0, 1.0], size=nper // rate + 3)
    ph = rng.uniform(-0.3, 0.3)
    for e in range(nper):
        d = sign[(e + off) // rate]
        II[e] = np.rint(32 * (amp * np.cos(ph) * d * shape + rng.normal(0, amp / 8, ntap))) / 32
        QQ[e] = np.rint(32 * (amp * np.sin(ph) * d * shape + rng.normal(0, amp / 8, ntap))) / 32
        if e >= first_sync:
            fs[e] = 1
            if (e + off) % rate == rate - 1:
                nb[e] = int(d) if rng.random() > 0.1 else -int(d)
    if extra_end is not None and nb[extra_end] == 0 and fs[extra_end]:
        nb[extra_end] = 1
    return II, QQ, fs, nb


def _junk_state(rng):
    st = cr.zero_state()
    for f in cr.TAPS + cr.PAIRS:
        st[f][:] = rng.normal(0, 1e6, len(st[f]))
    st.update(win_cnt=901, open=1, n=1, k=0, bits=5, nbad=1, alarm=1, alarms=3, windows=4, worst_pair=2)
    return st


def _case(gc, corrn, seed):
    rng = np.random.default_rng(seed)
    ntap = 1 + 2 * corrn
    II, QQ = np.zeros((NCH, NPER, ntap)), np.zeros((NCH, NPER, ntap))
    log = np.zeros((NCH, NPER), dtype=np.dtype(gc.TrkLog))
    for f in ("carrfreq", "codefreq", "remcode", "remcarr"):          # columns the monitor must not read
        log[f] = rng.normal(size=(NCH, NPER))
    for i, r in enumerate(RATES):
        II[i], QQ[i], log["flagsync"][i], log["navbit"][i] = _rows(rng, NPER, r, ntap, first_sync=[3, 0, 5, 0, 0][i],
                                                                   extra_end=[90, None, 33, None, None][i])
    ndone = np.array(NDONE, np.int32)
    for i in range(NCH):                                                # behind ndone: rows that would poison any sum
        II[i, ndone[i]:] = np.nan
        QQ[i, ndone[i]:] = np.inf
        log["flagsync"][i, ndone[i]:] = 1
        log["navbit"][i, ndone[i]:] = 1
    cnt0 = np.array(CNT0, np.uint64)
    prms = [cr.prm(kbits=[2, 1, 3, 1, 1][i], skip_bits=[1, 0, 2, 0, 0][i], nbad=[1, 2, 2, 1, 1][i], npair=[corrn, 1, corrn, 1, 1][i],
                   dtol=[0.02, 0.05, 0.01, 0.1, 0.1][i], rtol=[0.02, 0.05, 0.01, 0.1, 0.1][i],
                   dref=np.zeros(corrn), rref=[max(0.0, 2.0 - j) if j <= 2 else 0.0 for j in range(1, corrn + 1)]) for i in range(NCH)]
    st = [_junk_state(rng) if i in (0, 1, 3) else cr.zero_state() for i in range(NCH)]      # 0: reset by cnt0 == 0; 1, 3: carried on
    return prms, II, QQ, log, ndone, cnt0, st


def _restate(corrn, prms, II, QQ, log, ndone, cnt0, st, rates=RATES):
    return [cr.run(cr.copy_state(st[i]), prms[i], rates[i], corrn, II[i], QQ[i], log["flagsync"][i], log["navbit"][i], int(ndone[i]),
                   int(cnt0[i])) for i in range(len(st))]


def _structs(gc, prms, st):
    parr = np.zeros(len(prms), dtype=np.dtype(gc.CfmPrm))
    sarr = np.zeros(len(st), dtype=np.dtype(gc.CfmState))
    for i in range(len(prms)):
        cr.to_prm_struct(prms[i], parr[i])
        cr.to_struct(st[i], sarr[i])
    return parr, sarr


def _device(gc, eng, corrn, prms, II, QQ, log, ndone, cnt0, st, rates=RATES):
    parr, sarr = _structs(gc, prms, st)
    return eng.cfm_run(parr, rates[:len(st)], corrn, sarr, II, QQ, log, ndone, cnt0)


def _assert_same(want, got):
    for i, w in enumerate(want):
        assert cr.same(w, got[i]) == [], (i, cr.same(w, got[i])[:4])


@pytest.mark.parametrize("corrn", CORRNS)
def test_cfm_run_equals_restatement(gc, eng, corrn):
    case = _case(gc, corrn, seed=100 + corrn)
    want = _restate(corrn, *case)
    got = _device(gc, eng, corrn, *case)
    _assert_same(want, got)
    # what the case is for
    w0, w1, w2, w3, w4 = want
    # 0: reset by cnt0 == 0 (nothing of the junk's 4 windows); six bit ends at the least, the first opens, the extra end
    #    at row 90 costs a bit: four whole bits or five
    assert 1 <= w0["windows"] <= 2 and 4 <= w0["bits"] <= 5 and w0["win_cnt"] < NPER
    # 1: carried on from the junk's 4 windows and 5 bits: six bit ends in 65 rows, five whole bits at the least
    assert w1["windows"] >= 4 + 5 and w1["win_cnt"] > 1 << 32 and w1["bits"] >= 5 + 5
    assert w2["windows"] >= 8 and w2["alarms"] >= 1 and w2["bits"] >= 26
    assert (w3["windows"], w3["bits"]) in ((4, 5), (5, 6))              # one row: it closes the junk's open bit, or not
    assert cr.same(case[-1][4], got[4]) == []                                                           # no row: untouched
    assert {w["worst_pair"] for w in want[:3]} != {0}
    for _ in range(2):                                                   # and from run to run
        assert _device(gc, eng, corrn, *case).tobytes() == got.tobytes()


@pytest.mark.parametrize("corrn", [2, 16])
def test_cfm_run_cut_at_every_row_of_a_bit(gc, eng, corrn):
    """All rows of all channels in one call, and in two calls cut at every row of the rate-20 bit that straddles the
    chunk boundary at row 64 (before its first row to behind its last), the state threaded through."""
    prms, II, QQ, log, ndone, cnt0, st = _case(gc, corrn, seed=200 + corrn)
    rng = np.random.default_rng(9)
    ntap = 1 + 2 * corrn
    for i, r in enumerate(RATES):
        II[i], QQ[i], log["flagsync"][i], log["navbit"][i] = _rows(rng, NPER, r, ntap, first_sync=2 * i)
    ndone[:] = NPER
    whole = _device(gc, eng, corrn, prms, II, QQ, log, ndone, cnt0, st)
    _assert_same(_restate(corrn, prms, II, QQ, log, ndone, cnt0, st), whole)
    ends = np.flatnonzero(log["navbit"][0])
    last = int(ends[ends >= 64][0])
    first = last - RATES[0] + 1
    assert first <= 63 < 64 <= last and log["navbit"][0, first - 1] != 0                                  # the bit straddles the chunks
    for cut in range(first, last + 2):
        a = _device(gc, eng, corrn, prms, II[:, :cut], QQ[:, :cut], log[:, :cut], np.full(NCH, cut, np.int32), cnt0, st)
        mid = [cr.from_struct(x) for x in a]
        b = _device(gc, eng, corrn, prms, II[:, cut:], QQ[:, cut:], log[:, cut:], np.full(NCH, NPER - cut, np.int32),
                    cnt0 + np.uint64(cut), mid)
        assert b.tobytes() == whole.tobytes(), cut
    assert all(int(whole[i]["windows"]) >= 1 for i in range(NCH))


def test_cfm_run_leaves_a_channel_that_is_off_untouched(gc, eng):
    corrn = 2
    prms, II, QQ, log, ndone, cnt0, st = _case(gc, corrn, seed=31)
    ndone[:] = NPER
    II, QQ = np.nan_to_num(II, nan=1.0), np.nan_to_num(QQ, posinf=2.0)
    prms[2] = cr.prm()                                                   # kbits 0 between live channels
    st[2] = _junk_state(np.random.default_rng(1))
    parr, sarr = _structs(gc, prms, st)
    sarr["pad"][2] = 77
    before = sarr[2].tobytes()
    got = eng.cfm_run(parr, RATES, corrn, sarr, II, QQ, log, ndone, cnt0)
    assert got[2].tobytes() == before
    want = _restate(corrn, prms, II, QQ, log, ndone, cnt0, st)
    for i in (0, 1, 3, 4):
        assert cr.same(want[i], got[i]) == [], i
    assert want[0]["windows"] >= 1 and want[1]["windows"] > 4


BAD = [("kbits", -1), ("kbits", 4097), ("skip_bits", -1), ("nbad", 0), ("npair", 0), ("npair", 3), ("dtol", 0.0), ("dtol", float("nan")),
       ("rtol", -1.0), ("rtol", float("nan")), ("dref", float("inf")), ("dref", float("nan")), ("rref", float("-inf")),
       ("rref", float("nan")), ("rate", 1), ("rate", 21), ("ndone", -1), ("ndone", NPER + 1)]


@pytest.mark.parametrize("field,value", BAD)
def test_cfm_run_refusals_name_the_channel_and_the_field_and_touch_nothing(gc, eng, field, value):
    corrn = 2
    prms, II, QQ, log, ndone, cnt0, st = _case(gc, corrn, seed=9)
    rates = list(RATES)
    if field == "rate":
        rates[1] = value
    elif field == "ndone":
        ndone[1] = value
    elif field in ("dref", "rref"):
        prms[1][field][15] = value                                       # beyond npair, beyond corrn: still refused
    else:
        prms[1][field] = value
    parr, sarr = _structs(gc, prms, st)
    before = sarr.tobytes()
    with pytest.raises(gc.GnsscorrError) as ei:
        eng.cfm_run(parr, rates, corrn, sarr, II, QQ, log, ndone, cnt0)
    assert field in str(ei.value) and "channel 1" in str(ei.value)
    assert sarr.tobytes() == before


def test_cfm_run_null_shape_and_corrn_errors(gc, eng):
    corrn = 2
    prms, II, QQ, log, ndone, cnt0, st = _case(gc, corrn, seed=9)
    parr, sarr = _structs(gc, prms, st)
    before = sarr.tobytes()
    rates = np.asarray(RATES, np.int32)
    L = gc.lib()
    ptr = [parr.ctypes.data, rates.ctypes.data, sarr.ctypes.data, II.ctypes.data, QQ.ctypes.data, log.ctypes.data, ndone.ctypes.data,
           cnt0.ctypes.data]
    call = lambda h, a, c, nch, nper: L.gnsscorr_cfm_run(h, a[0], a[1], c, *a[2:], nch, nper)
    assert call(eng.h, ptr, corrn, NCH, 0) == -1 and call(eng.h, ptr, corrn, -1, NPER) == -1
    assert call(eng.h, ptr, 0, NCH, NPER) == -1 and call(eng.h, ptr, 17, NCH, NPER) == -1
    for k in range(8):
        a = list(ptr)
        a[k] = None
        assert call(eng.h, a, corrn, NCH, NPER) == -1, k
    assert call(None, ptr, corrn, NCH, NPER) == -1 and sarr.tobytes() == before
    assert call(eng.h, ptr, corrn, 0, NPER) == 0
