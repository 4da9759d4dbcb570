"""The bit-synchronisation detector's kernel through its op-level seam (-m gpu): gnsscorr_bsync_run against the restated
rules (tests/bsync_restate.py) on crafted streams, every field of gnsscorr_bsync_t bit for bit.  The kernel takes the rows
in chunks of 64 and lane o owns offset o, so the row counts sit on both sides of one, two and four chunks and of a
symbol, and the rates run from 2 (two lanes) to 20 (every array element)."""
import numpy as np
import pytest

import bsync_restate as br

pytestmark = pytest.mark.gpu
RATES = [20, 10, 7, 3, 2, 20]
NPERS = [1, 19, 20, 21, 63, 64, 65, 128, 257]
MODES = ["first", "last", "behind", "zero", "early"]
CNT0 = 1000


@pytest.fixture(scope="module")
def eng(gc):
    e = gc.Engine(0)
    yield e
    e.close()


def _prompts(rng, n, rate, amp=2 ** 22):
    """Symbols of `rate` rows at a random alignment plus noise of the same size, in multiples of 1/32 up to about 2^23:
    the squares of the symbol sums do not fit a double, so every rounding counts."""
    sym = rng.choice([-1.0, 1.0], size=n // rate + 2)
    off = int(rng.integers(0, rate))
    s = sym[(np.arange(n) + off) // rate]
    ph = rng.uniform(0, 2 * np.pi)
    I = np.rint(32 * (amp * np.cos(ph) * s + rng.normal(0, amp, n))) / 32.0
    Q = np.rint(32 * (amp * np.sin(ph) * s + rng.normal(0, amp, n))) / 32.0
    return I, Q


def _junk_state(rng):
    st = br.zero_state()
    for f in ("E", "sI", "sQ"):
        st[f] = [float(x) for x in rng.normal(0, 1e6, br.NOFF)]
    st["fill"] = [int(x) for x in rng.integers(0, 2, br.NOFF)]
    st.update(ratio_last=3.25, a0=77, decided_cnt=901, armed=1, n=9, tests=4, done=2, best=3, synci=2)
    return st


def _case(gc, nper, mode, seed):
    """Six channels: 0-4 the five rates; 3 with ndone < nper and junk behind; 5 (rate 20) with flagsync rising in
    mid-stream.  mode: where start_cnt lies against the run (its first row, its last row, behind it, before it), or
    `zero`: cnt0 = 0 in front of a carried state."""
    rng = np.random.default_rng(seed)
    nch = len(RATES)
    I, Q = np.zeros((nch, nper)), np.zeros((nch, nper))
    for i, r in enumerate(RATES):
        I[i], Q[i] = _prompts(rng, nper, r)
    log = np.zeros((nch, nper), dtype=np.dtype(gc.TrkLog))
    for f in ("carrfreq", "codefreq", "remcode", "remcarr"):          # columns the detector must not read
        log[f] = rng.normal(size=(nch, nper))
    log["navbit"] = rng.integers(-1, 2, (nch, nper))
    log["flagsync"][5, nper // 2:] = 1
    ndone = np.full(nch, nper, np.int32)
    ndone[3] = nper * 2 // 3
    I[3, ndone[3]:] = np.nan
    Q[3, ndone[3]:] = np.inf
    log["flagsync"][3, ndone[3]:] = 1
    cnt0 = np.full(nch, 0 if mode == "zero" else CNT0, np.uint64)
    prm = np.zeros(nch, dtype=np.dtype(gc.BsyncPrm))
    prm["start_cnt"] = {"first": CNT0, "last": CNT0 + nper - 1, "behind": CNT0 + nper + 5, "zero": 0, "early": 3}[mode]
    prm["nsym"] = [2, 3, 4, 5, 7, 2]
    prm["nsym_max"] = [6, 9, 12, 40, 70, 6]
    prm["gate"] = [1.5, 1.5, 1.25, 1.25, 1.1, 1.5]
    st = [_junk_state(rng) if mode == "zero" else br.zero_state() for _ in range(nch)]
    return prm, I, Q, log, ndone, cnt0, st


def _prm_dict(p):
    return dict(start_cnt=int(p["start_cnt"]), nsym=int(p["nsym"]), nsym_max=int(p["nsym_max"]), gate=float(p["gate"]))


def _restate(prm, I, Q, log, ndone, cnt0, st, rates=RATES):
    return [br.run(br.copy_state(st[i]), _prm_dict(prm[i]), rates[i], I[i], Q[i], log["flagsync"][i], int(ndone[i]), int(cnt0[i]))
            for i in range(len(st))]


def _device(gc, eng, prm, I, Q, log, ndone, cnt0, st, rates=RATES):
    arr = np.zeros(len(st), dtype=np.dtype(gc.BsyncState))
    for i, s in enumerate(st):
        br.to_struct(s, arr[i])
    return eng.bsync_run(prm, rates[:len(st)], arr, I, Q, log, ndone, cnt0)


def _assert_same(want, got):
    for i, w in enumerate(want):
        assert br.same(w, got[i]) == [], (i, w, br.from_struct(got[i]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nper", NPERS)
def test_bsync_run_equals_restatement(gc, eng, nper, mode):
    case = _case(gc, nper, mode, seed=1000 * NPERS.index(nper) + MODES.index(mode))
    want = _restate(*case)
    _assert_same(want, _device(gc, eng, *case))
    # what the case is for
    ran = [i for i in range(len(RATES)) if case[4][i] > 0]
    if mode == "behind":
        assert all(w["armed"] == 0 and w["tests"] == 0 for w in want) and want[5]["done"] == 3    # (rule 3 before rule 4)
    if mode == "last" and nper > 1:
        assert all((w["armed"], w["a0"]) == (1, CNT0 + nper - 1) for w in want[:3]) and want[5]["done"] == 3
    if mode == "first":
        assert all((want[i]["armed"], want[i]["a0"]) == (1, CNT0) for i in ran if i != 5)
    if mode == "zero":
        assert all(want[i]["decided_cnt"] != 901 and want[i]["a0"] == 0 and want[i]["ratio_last"] != 3.25 for i in ran)
    if mode in ("first", "early", "zero") and nper == 257:
        assert want[0]["tests"] >= 1 and want[4]["tests"] >= 1
        assert sum(w["done"] == 1 for w in want) >= 2                   # the symbols are found


def test_bsync_run_cut_invariance_and_frozen_state(gc, eng):
    """The 257-row streams in one call and in pieces of 1, 63, 64, 65 and 64 rows with the state carried: identical
    states.  Then a finished channel stays frozen whatever it is fed, until a run whose row 0 has cnt == 0."""
    prm, I, Q, log, ndone, cnt0, st = _case(gc, 257, "early", seed=77)
    ndone[3] = 257
    I[3], Q[3] = _prompts(np.random.default_rng(5), 257, 3)
    log["flagsync"][3] = 0
    prm["nsym_max"][:] = [4096, 4096, 4096, 4096, 4096, 6]
    prm["gate"][1] = 1e9                                                # channel 1 keeps testing to the end
    whole = _device(gc, eng, prm, I, Q, log, ndone, cnt0, st)
    want = _restate(prm, I, Q, log, ndone, cnt0, st)
    _assert_same(want, whole)
    assert want[1]["done"] == 0 and want[1]["tests"] == 8
    cur, at = st, 0
    for n in (1, 63, 64, 65, 64):
        sl = slice(at, at + n)
        out = _device(gc, eng, prm, I[:, sl], Q[:, sl], log[:, sl], np.full(6, n, np.int32), cnt0 + np.uint64(at), cur)
        cur = [br.from_struct(x) for x in out]
        at += n
    assert at == 257 and out.tobytes() == whole.tobytes()
    done = [i for i in range(6) if whole[i]["done"]]
    assert len(done) >= 3 and 5 in done
    again = _device(gc, eng, prm, I, Q, log, ndone, cnt0 + np.uint64(257), cur)
    for i in done:
        assert again[i].tobytes() == whole[i].tobytes(), i
    fresh = _device(gc, eng, prm, I, Q, log, ndone, np.zeros(6, np.uint64), cur)
    _assert_same(_restate(prm, I, Q, log, ndone, np.zeros(6, np.uint64), cur), fresh)
    assert all(int(fresh[i]["a0"]) == 3 for i in range(5))
    for _ in range(2):                                                   # and from run to run
        assert _device(gc, eng, prm, I, Q, log, ndone, cnt0, st).tobytes() == whole.tobytes()


def test_bsync_run_gives_up_at_nsym_max_or_passes_at_the_second_test(gc, eng):
    """Rate 10: five and a half symbols of rows that cancel in every alignment (+1, -1, ...: every E stays 0, the test
    at n = 4 fails with ratio 0), then alternating symbols.  nsym_max 4: given up there.  nsym_max 8: the test at
    n = 8 passes on the layout's edge."""
    R, nper, cnt0 = 10, 100, 500
    p0 = 7                                                               # row e holds period p0 + e of symbol (p0 + e) // R
    e = np.arange(nper)
    I = np.where(e < 55, np.where(e % 2 == 0, 1.0, -1.0), np.where(((p0 + e) // R) % 2 == 0, 5.0, -5.0))
    I = np.stack([I, I])
    Q = np.zeros((2, nper))
    log = np.zeros((2, nper), dtype=np.dtype(gc.TrkLog))
    prm = np.zeros(2, dtype=np.dtype(gc.BsyncPrm))
    prm["start_cnt"], prm["nsym"], prm["nsym_max"], prm["gate"] = 0, 4, [4, 8], 2.0
    args = (prm, I, Q, log, np.full(2, nper, np.int32), np.full(2, cnt0, np.uint64), [br.zero_state(), br.zero_state()])
    want = _restate(*args, rates=[R, R])
    got = _device(gc, eng, *args, rates=[R, R])
    _assert_same(want, got)
    g = [br.from_struct(x) for x in got]
    assert (g[0]["done"], g[0]["tests"], g[0]["n"], g[0]["ratio_last"], g[0]["decided_cnt"]) == (2, 1, 4, 0.0, 0)
    assert all(x == 0.0 for x in g[0]["E"])
    synci = br.layout_synci(p0, cnt0, R)
    assert (g[1]["done"], g[1]["tests"], g[1]["n"], g[1]["synci"], g[1]["best"]) == (1, 2, 8, synci, (synci + 1) % R)
    assert g[1]["decided_cnt"] == cnt0 + 9 * R - 2


def test_bsync_run_equal_maxima_take_the_lowest_offset(gc, eng):
    """Integer prompts whose energies tie: constant rows (all four offsets equal: offset 0, and gate 1 passes on the
    tie with the half-symbol alignment) and a triangle wave of two symbols' length (two equal maxima next to each other)."""
    R, nper = 4, 40
    tri = np.array([2.0, 1.0, 0.0, -1.0, -2.0, -1.0, 0.0, 1.0])
    for cnt0 in (400, 401, 402, 403):
        I = np.stack([np.ones(nper), tri[(np.arange(nper) + cnt0) % 8]])
        Q = np.zeros((2, nper))
        log = np.zeros((2, nper), dtype=np.dtype(gc.TrkLog))
        prm = np.zeros(2, dtype=np.dtype(gc.BsyncPrm))
        prm["start_cnt"], prm["nsym"], prm["nsym_max"], prm["gate"] = 0, 4, 4, 1.0
        args = (prm, I, Q, log, np.full(2, nper, np.int32), np.full(2, cnt0, np.uint64), [br.zero_state(), br.zero_state()])
        want = _restate(*args, rates=[R, R])
        got = _device(gc, eng, *args, rates=[R, R])
        _assert_same(want, got)
        g = [br.from_struct(x) for x in got]
        assert g[0]["E"][:4] == [64.0] * 4 and (g[0]["done"], g[0]["best"], g[0]["synci"], g[0]["ratio_last"]) == (1, 0, 3, 1.0)
        E = g[1]["E"][:4]
        assert sorted(E) == [16.0, 16.0, 64.0, 64.0] and g[1]["best"] == E.index(64.0) and g[1]["done"] == 1, (cnt0, E)


def test_bsync_run_gate_is_a_product_and_not_strict(gc, eng):
    """Rate 2, rows 2, 1, 1, 0 repeating: the symbol sums are 3 and 1 at one alignment and 2 and 2 at the other, so
    after four symbols E = 20 against 16.  gate = 1.25 passes (20 >= 1.25 * 16 exactly); one ulp more does not."""
    R, nper, cnt0 = 2, 10, 64
    I = np.array([2.0, 1.0, 1.0, 0.0] * 3)[None, :nper]
    Q = np.zeros((1, nper))
    log = np.zeros((1, nper), dtype=np.dtype(gc.TrkLog))
    prm = np.zeros(1, dtype=np.dtype(gc.BsyncPrm))
    prm["start_cnt"], prm["nsym"], prm["nsym_max"] = 0, 4, 4
    for gate, done in ((1.25, 1), (float(np.nextafter(1.25, 2.0)), 2)):
        prm["gate"] = gate
        args = (prm, I, Q, log, np.full(1, nper, np.int32), np.full(1, cnt0, np.uint64), [br.zero_state()])
        want = _restate(*args, rates=[R])
        got = _device(gc, eng, *args, rates=[R])
        _assert_same(want, got)
        g = br.from_struct(got[0])
        assert (g["E"][:2], g["done"], g["tests"], g["ratio_last"]) == ([20.0, 16.0], done, 1, 1.25), (gate, g)
        if done == 1:
            assert (g["best"], g["synci"], g["decided_cnt"]) == (0, 1, cnt0 + 8)


def test_bsync_run_33_channels_of_mixed_rates_some_off(gc, eng):
    """More channels than a workgroup holds, of every rate from 2 to 20 with their own parameters and row counts; every
    fourth has the detector off and keeps its (junk) state to the byte."""
    rng = np.random.default_rng(33)
    nch, nper = 33, 150
    rates = [int(r) for r in rng.integers(2, 21, nch)]
    rates[:5] = [20, 2, 13, 5, 19]
    I, Q = np.zeros((nch, nper)), np.zeros((nch, nper))
    for i, r in enumerate(rates):
        I[i], Q[i] = _prompts(rng, nper, r)
    log = np.zeros((nch, nper), dtype=np.dtype(gc.TrkLog))
    log["flagsync"][7, 100:] = 1
    ndone = rng.integers(0, nper + 1, nch).astype(np.int32)
    ndone[:8] = nper
    cnt0 = rng.integers(0, 3000, nch).astype(np.uint64)
    cnt0[2] = 0
    prm = np.zeros(nch, dtype=np.dtype(gc.BsyncPrm))
    prm["start_cnt"] = rng.integers(0, 3100, nch)
    prm["start_cnt"][:8] = 0
    prm["nsym"] = rng.integers(1, 4, nch)
    prm["nsym_max"] = prm["nsym"] * rng.integers(1, 5, nch)
    prm["gate"] = rng.choice([1.0, 1.25, 1.5, 3.0], nch)
    off = list(range(3, nch, 4))
    prm["nsym"][off] = 0
    st = [_junk_state(rng) if i in off or i == 2 else br.zero_state() for i in range(nch)]
    want = _restate(prm, I, Q, log, ndone, cnt0, st, rates=rates)
    arr = np.zeros(nch, dtype=np.dtype(gc.BsyncState))
    for i, s in enumerate(st):
        br.to_struct(s, arr[i])
    before = [arr[i].tobytes() for i in range(nch)]
    got = eng.bsync_run(prm, rates, arr, I, Q, log, ndone, cnt0)
    _assert_same(want, got)
    assert all(got[i].tobytes() == before[i] for i in off)
    assert sum(w["done"] == 1 for w in want) >= 5 and sum(w["done"] == 2 for i, w in enumerate(want) if i not in off) >= 1
    assert want[7]["done"] in (1, 2, 3) and want[2]["a0"] == 0


@pytest.mark.parametrize("field,value,word", [
    ("start_cnt", -1, "start_cnt"), ("nsym", -1, "nsym"), ("nsym", 10, "nsym"), ("nsym_max", 4097, "nsym_max"),
    ("nsym_max", 0, "nsym_max"), ("gate", 0.999, "gate"), ("gate", float("nan"), "gate"),
    ("rate", 1, "rate"), ("rate", 21, "rate"), ("ndone", 22, "ndone"), ("ndone", -1, "ndone")])
def test_bsync_run_parameter_errors_leave_the_state_untouched(gc, eng, field, value, word):
    prm, I, Q, log, ndone, cnt0, st = _case(gc, 21, "first", seed=9)
    rates = list(RATES)
    if field == "rate":
        rates[1] = value
    elif field == "ndone":
        ndone[1] = value
    else:
        prm[field][1] = value
    arr = np.zeros(6, dtype=np.dtype(gc.BsyncState))
    for i, s in enumerate(st):
        br.to_struct(s, arr[i])
    before = arr.tobytes()
    with pytest.raises(gc.GnsscorrError) as ei:
        eng.bsync_run(prm, rates, arr, I, Q, log, ndone, cnt0)
    assert word in str(ei.value) and "channel 1" in str(ei.value)
    assert arr.tobytes() == before


def test_bsync_run_null_and_shape_errors(gc, eng):
    prm, I, Q, log, ndone, cnt0, st = _case(gc, 21, "first", seed=9)
    arr = np.zeros(6, dtype=np.dtype(gc.BsyncState))
    before = arr.tobytes()
    rates = np.asarray(RATES, np.int32)
    L = gc.lib()
    args = [prm.ctypes.data, rates.ctypes.data, arr.ctypes.data, I.ctypes.data, Q.ctypes.data, log.ctypes.data, ndone.ctypes.data,
            cnt0.ctypes.data]
    assert L.gnsscorr_bsync_run(eng.h, *args, 6, 0) == -1 and L.gnsscorr_bsync_run(eng.h, *args, -1, 21) == -1
    for k in range(8):
        a = list(args)
        a[k] = None
        assert L.gnsscorr_bsync_run(eng.h, *a, 6, 21) == -1, k
    assert L.gnsscorr_bsync_run(None, *args, 6, 21) == -1 and arr.tobytes() == before
    assert L.gnsscorr_bsync_run(eng.h, *args, 0, 21) == 0
