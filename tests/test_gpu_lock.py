"""The lock monitor's kernel through its op-level seam (-m gpu): gnsscorr_lock_run against the restated detector
(tests/lock_restate.py) on crafted streams, every field of gnsscorr_lock_t bit for bit.  The kernel takes the rows in
chunks of 64, so the row counts sit on both sides of one, two and four chunks and of a nav bit; rate 2 puts a bit end on
every second lane."""
import ctypes as C

import numpy as np
import pytest

import lock_restate as lr

pytestmark = pytest.mark.gpu
RATES = [20, 10, 2, 20, 20]
NPERS = [1, 19, 20, 21, 63, 64, 65, 128, 257]
CNT_MODES = ["zero", "five", "timeout_first", "timeout_last"]
SYNC_PERIODS = 1000


@pytest.fixture(scope="module")
def eng(gc):
    e = gc.Engine(0)
    yield e
    e.close()


def _noise(rng, n):
    """Random multiples of 1/32 up to +-2^20: the squares of the bit sums do not fit a double, so every rounding counts."""
    return rng.integers(-2 ** 25, 2 ** 25 + 1, n) / 32.0


def _edges(rng, n, rate):
    nb = np.zeros(n, np.int32)
    idx = np.arange(int(rng.integers(0, rate)), n, rate)
    nb[idx] = rng.choice([-1, 1], size=idx.size)
    return nb


def _carried(rng, lost=0):
    st = lr.zero_state()
    st.update(open=1, n=3, sI=float(_noise(rng, 1)[0]), sQ=float(_noise(rng, 1)[0]), w=float(abs(_noise(rng, 1)[0])) * 2.0 ** 20,
              k=1, npsum=1.5, nbad=1, windows=7, mu_last=0.75)
    if lost:
        st.update(lost=1, reason=2, lost_cnt=123)
    return st


def _case(gc, nper, mode, seed):
    """Five channels: 0 noise, flagsync rising mid-stream, one irregular bit; 1 constant signal; 2 noise at rate 2;
    3 noise with ndone < nper and junk behind; 4 never synchronised, against the time limit."""
    rng = np.random.default_rng(seed)
    nch = len(RATES)
    I = np.stack([_noise(rng, nper) for _ in range(nch)])
    Q = np.stack([_noise(rng, nper) for _ in range(nch)])
    log = np.zeros((nch, nper), dtype=np.dtype(gc.TrkLog))
    for f in ("carrfreq", "codefreq", "remcode", "remcarr"):          # columns the monitor must not read
        log[f] = rng.normal(size=(nch, nper))
    log["flagloopfilter"] = 2
    for i, r in enumerate(RATES):
        log["navbit"][i] = _edges(rng, nper, r)
        log["flagsync"][i] = 1
    log["flagsync"][0, :nper // 3] = 0
    if nper > 40:
        log["navbit"][0, nper // 2 + 3] = -1                            # an irregular bit (whichever way it cuts)
        log["navbit"][0, nper // 2 + 4] = 1
    I[1], Q[1] = 1.0, 0.0
    log["flagsync"][4] = 0
    log["navbit"][4] = _edges(rng, nper, 20)                            # (decided bits without synchronisation count for nothing)
    ndone = np.full(nch, nper, np.int32)
    ndone[3] = nper * 2 // 3
    I[3, ndone[3]:] = np.nan
    Q[3, ndone[3]:] = np.inf
    log["flagsync"][3, ndone[3]:] = rng.integers(0, 2, nper - ndone[3])
    log["navbit"][3, ndone[3]:] = rng.integers(-1, 2, nper - ndone[3])
    cnt0 = {"zero": 0, "five": 5, "timeout_first": SYNC_PERIODS - 1, "timeout_last": SYNC_PERIODS - nper}[mode]
    cnt0 = np.full(nch, cnt0, np.uint64)
    prm = np.zeros(nch, dtype=np.dtype(gc.LockPrm))
    prm["sync_periods"], prm["nbad"] = SYNC_PERIODS, 2
    prm["kbits"] = [2, 3, 10, 1, 2]
    prm["mu_min"] = [1.0, 9.5, 1.0, 1.0, 1.0]                           # noise: np is about 1, so about every other window is bad
    st = [_carried(rng, lost=(mode == "zero" and i % 2 == 0)) for i in range(nch)]
    return prm, I, Q, log, ndone, cnt0, st


def _restate(prm, I, Q, log, ndone, cnt0, st, rates=RATES):
    out = []
    for i, r in enumerate(rates[:len(st)]):
        p = dict(sync_periods=int(prm[i]["sync_periods"]), kbits=int(prm[i]["kbits"]), nbad=int(prm[i]["nbad"]),
                 mu_min=float(prm[i]["mu_min"]))
        out.append(lr.run(dict(st[i]), p, r, I[i], Q[i], log["flagsync"][i], log["navbit"][i], int(ndone[i]), int(cnt0[i])))
    return out


def _device(gc, eng, prm, I, Q, log, ndone, cnt0, st, rates=RATES):
    arr = np.zeros(len(st), dtype=np.dtype(gc.LockState))
    for i, s in enumerate(st):
        lr.to_struct(s, arr[i])
    return eng.lock_run(prm, rates[:len(st)], arr, I, Q, log, ndone, cnt0)


@pytest.mark.parametrize("mode", CNT_MODES)
@pytest.mark.parametrize("nper", NPERS)
def test_lock_run_equals_restatement(gc, eng, nper, mode):
    case = _case(gc, nper, mode, seed=1000 * NPERS.index(nper) + CNT_MODES.index(mode))
    want = _restate(*case)
    got = _device(gc, eng, *case)
    for i in range(len(RATES)):
        assert lr.same(want[i], got[i]) == [], (i, want[i], lr.from_struct(got[i]))
    # what the case is for
    if mode == "timeout_first":
        assert (want[4]["lost"], want[4]["reason"], want[4]["lost_cnt"]) == (1, 1, SYNC_PERIODS - 1)
    if mode == "timeout_last":
        assert (want[4]["lost"], want[4]["reason"], want[4]["lost_cnt"]) == (1, 1, SYNC_PERIODS - 1)
        if nper > 1:
            assert want[0]["lost"] == 0 or want[0]["reason"] == 2      # it synchronised before the limit
    if mode == "five":
        assert want[4]["lost"] == 0
    if mode == "zero":
        assert all(w["lost_cnt"] != 123 for w in want)                  # the lost states were reset
        assert want[1]["lost"] == 0 and (nper < 60 or want[1]["mu_last"] == 10.0)
    else:
        assert nper < 60 or want[1]["windows"] > 7
    if nper == 257 and mode == "five":
        assert want[2]["windows"] >= 7 + 12 or want[2]["lost"]
        assert any(w["reason"] == 2 for w in want)                      # the power rule fires somewhere


def test_lock_run_hand_streams(gc, eng):
    """Constant signal: np == rate exactly; alternating signs: np == 0; all-zero rows: np = 0 by the w > 0 rule; a bit
    of 7 periods is dropped.  Against the restatement and against the answers known by hand."""
    nper, rates = 257, [20, 20, 20, 20]
    I = np.zeros((4, nper))
    Q = np.zeros((4, nper))
    alt = np.where(np.arange(nper) % 2 == 0, 1.0, -1.0)
    I[0], I[1], Q[1], I[3] = 1.0, alt, -alt, 1.0
    log = np.zeros((4, nper), dtype=np.dtype(gc.TrkLog))
    log["flagsync"] = 1
    log["navbit"][:, 10::20] = 1
    log["navbit"][3, 37] = -1
    prm = np.zeros(4, dtype=np.dtype(gc.LockPrm))
    prm["kbits"], prm["nbad"], prm["mu_min"] = [3, 2, 2, 1], [2, 3, 3, 100], [20.0, 1.0, 1.0, 1.0]
    ndone, cnt0 = np.full(4, nper, np.int32), np.full(4, 5, np.uint64)
    st = [lr.zero_state() for _ in range(4)]
    want = _restate(prm, I, Q, log, ndone, cnt0, st, rates=rates)
    got = _device(gc, eng, prm, I, Q, log, ndone, cnt0, st, rates=rates)
    for i in range(4):
        assert lr.same(want[i], got[i]) == [], (i, want[i], lr.from_struct(got[i]))
    g = [lr.from_struct(x) for x in got]
    assert (g[0]["windows"], g[0]["mu_last"], g[0]["lost"], g[0]["nbad"]) == (4, 20.0, 0, 0)     # mu == mu_min is not bad
    for x in g[1:3]:
        assert (x["lost"], x["reason"], x["lost_cnt"], x["mu_last"], x["windows"]) == (1, 2, 5 + 130, 0.0, 3)
    assert (g[3]["windows"], g[3]["mu_last"], g[3]["lost"]) == (11, 20.0, 0)                    # 14 bits closed, 3 of them not whole
    # a weaker period in the first whole bit: its np, and so the first window's mean, falls below 20
    prm["nbad"][0] = 1
    I[0, 15] = 0.5
    want = _restate(prm, I, Q, log, ndone, cnt0, st, rates=rates)
    got = _device(gc, eng, prm, I, Q, log, ndone, cnt0, st, rates=rates)
    assert lr.same(want[0], got[0]) == []
    assert (int(got[0]["lost"]), int(got[0]["lost_cnt"]), int(got[0]["windows"])) == (1, 5 + 70, 1) and got[0]["mu_last"] < 20.0


def test_lock_run_threshold_is_strict(gc, eng):
    """mu == mu_min is not bad, mu_min one ulp above mu is: on noise, so that mu is no round number."""
    rng = np.random.default_rng(31)
    nper = 100
    I, Q = _noise(rng, nper)[None, :], _noise(rng, nper)[None, :]
    log = np.zeros((1, nper), dtype=np.dtype(gc.TrkLog))
    log["flagsync"] = 1
    log["navbit"][0, 0::20] = 1
    prm = np.zeros(1, dtype=np.dtype(gc.LockPrm))
    prm["kbits"], prm["nbad"], prm["mu_min"] = 2, 1, 1e-9
    args = (I, Q, log, np.full(1, nper, np.int32), np.full(1, 5, np.uint64), [lr.zero_state()])
    ev = []
    lr.run(lr.zero_state(), dict(sync_periods=0, kbits=2, nbad=1, mu_min=1e-9), 20, I[0], Q[0], log["flagsync"][0], log["navbit"][0],
           nper, 5, events=ev)
    mu = [e[2] for e in ev if e[0] == "mu"][0]
    assert 0.0 < mu < 20.0
    prm["mu_min"] = mu
    got = _device(gc, eng, prm, *args, rates=[20])
    assert lr.same(_restate(prm, *args, rates=[20])[0], got[0]) == [] and int(got[0]["lost"]) == 0 and int(got[0]["windows"]) == 2
    prm["mu_min"] = np.nextafter(mu, np.inf)
    got = _device(gc, eng, prm, *args, rates=[20])
    assert lr.same(_restate(prm, *args, rates=[20])[0], got[0]) == []
    assert (int(got[0]["lost"]), int(got[0]["reason"]), int(got[0]["lost_cnt"]), int(got[0]["windows"])) == (1, 2, 5 + 40, 1)
    assert got[0]["mu_last"] == mu


def test_lock_run_cut_invariance_and_frozen_state(gc, eng):
    """The 257-row streams in one call and in pieces of 1, 63, 64, 65 and 64 rows with the state carried: identical
    states.  Then a lost channel stays frozen whatever it is fed, until a run whose row 0 has cnt == 0."""
    prm, I, Q, log, ndone, cnt0, st = _case(gc, 257, "five", seed=77)
    ndone[3] = 257
    I[3], Q[3] = _noise(np.random.default_rng(5), 257), _noise(np.random.default_rng(6), 257)
    whole = _device(gc, eng, prm, I, Q, log, ndone, cnt0, st)
    want = _restate(prm, I, Q, log, ndone, cnt0, st)
    for i in range(5):
        assert lr.same(want[i], whole[i]) == [], i
    cur, at = st, 0
    for n in (1, 63, 64, 65, 64):
        sl = slice(at, at + n)
        out = _device(gc, eng, prm, I[:, sl], Q[:, sl], log[:, sl], np.full(5, n, np.int32), cnt0 + np.uint64(at), cur)
        cur = [lr.from_struct(x) for x in out]
        at += n
    assert at == 257
    assert out.tobytes() == whole.tobytes()
    assert sum(int(x["lost"]) for x in whole) >= 1
    # frozen
    lost = [i for i in range(5) if whole[i]["lost"]]
    again = _device(gc, eng, prm, I, Q, log, ndone, cnt0 + np.uint64(257), cur)
    for i in lost:
        assert again[i].tobytes() == whole[i].tobytes(), i
    # cnt0 == 0: the state starts over
    fresh = _device(gc, eng, prm, I, Q, log, ndone, np.zeros(5, np.uint64), cur)
    want0 = _restate(prm, I, Q, log, ndone, np.zeros(5, np.uint64), cur)
    for i in range(5):
        assert lr.same(want0[i], fresh[i]) == [], i
    assert all(int(fresh[i]["lost_cnt"]) < 257 for i in lost)


def test_lock_run_runs_are_bit_identical(gc, eng):
    case = _case(gc, 257, "five", seed=4242)
    a = _device(gc, eng, *case).tobytes()
    for _ in range(3):
        assert _device(gc, eng, *case).tobytes() == a


@pytest.mark.parametrize("field,value,word", [
    ("kbits", 0, "kbits"), ("kbits", 4097, "kbits"), ("nbad", 0, "nbad"), ("sync_periods", -1, "sync_periods"),
    ("mu_min", 0.0, "mu_min"), ("mu_min", 10.5, "mu_min"), ("mu_min", float("nan"), "mu_min"),
    ("rate", 1, "rate"), ("rate", 21, "rate"), ("ndone", 22, "ndone"), ("ndone", -1, "ndone")])
def test_lock_run_parameter_errors_leave_the_state_untouched(gc, eng, field, value, word):
    prm, I, Q, log, ndone, cnt0, st = _case(gc, 21, "five", seed=9)
    rates = list(RATES)
    if field == "rate":
        rates[1] = value
    elif field == "ndone":
        ndone[1] = value
    else:
        prm[field][1] = value
    arr = np.zeros(5, dtype=np.dtype(gc.LockState))
    for i, s in enumerate(st):
        lr.to_struct(s, arr[i])
    before = arr.tobytes()
    with pytest.raises(gc.GnsscorrError) as ei:
        eng.lock_run(prm, rates, arr, I, Q, log, ndone, cnt0)
    assert word in str(ei.value) and "channel 1" in str(ei.value)
    assert arr.tobytes() == before
    rc = gc.lib().gnsscorr_lock_run(eng.h, prm.ctypes.data, np.asarray(RATES, np.int32).ctypes.data, arr.ctypes.data, I.ctypes.data,
                                    Q.ctypes.data, log.ctypes.data, np.full(5, 1, np.int32).ctypes.data, cnt0.ctypes.data, 5, 0)
    assert rc == -1 and arr.tobytes() == before
