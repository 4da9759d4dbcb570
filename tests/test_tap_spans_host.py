"""The closed loop's code and carrier tables at wide tap spans, on the CPU: the host twins of gnsscorr_nco.h
(tests/host/nco_host.cpp) against the oracle's literal loops, over the cases of tests/tap_span_cases.py that
tests/test_gpu_tap_spans.py runs on the device.  No GPU.

What is shown here:
  - the map: at which outermost tap the shape-specialised code step's pieces stop fitting GC_NCODE, per sample rate;
  - that the cases named state-dependent hold periods on both sides of that boundary inside one channel's run;
  - that the ladder of the tail's table tasks (step, else walker; a step that overflowed its table counts as declined)
    gives the oracle's chip at every replica position, its LUT entry at every sample and both remainders, within
    GC_NCODE / GC_NCAR pieces, for every period of every case -- and that the ladder without the overflow rule does not."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tap_span_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "nco_host.cpp")
DPI = 2.0 * 3.1415926535897932
NCODE, NCAR = tc.header_const("GC_NCODE"), tc.header_const("GC_NCAR")


@pytest.fixture(scope="module")
def nco(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tapspans") / "nco_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    d, i, vp = C.c_double, C.c_int, C.c_void_p
    L.nco_code_period_pieces.argtypes = [d, d, i, d, i, i, C.POINTER(d)]
    L.nco_carrier_period_pieces.argtypes = [d, d, d, i, C.POINTER(d)]
    L.nco_tail_code_ladder.argtypes = [d, d, i, d, i, i, i, i, vp, C.POINTER(d), C.POINTER(i)]
    L.nco_tail_carrier_ladder.argtypes = [d, d, d, i, i, vp, C.POINTER(d), C.POINTER(i)]
    L.nco_carrier_fast.argtypes = [d, d, d, i, i, vp, C.POINTER(d)]
    return L


def _step_pieces(nco, f_sf, codefreq, remcode, span):
    n = tc.nsamp_ref(tc.CLEN, remcode, codefreq, f_sf)
    rem = C.c_double()
    return nco.nco_code_period_pieces(1.0 / f_sf, codefreq, tc.CLEN, remcode, span, n + 2 * span, C.byref(rem))


def _ladder(nco, f_sf, codefreq, remcode, span, give_up, chip=None):
    """-> (pieces or -1, rung, remainder, chips) of the tail's code ladder with GC_NCODE pieces of room."""
    n = tc.nsamp_ref(tc.CLEN, remcode, codefreq, f_sf)
    nt = n + 2 * span
    chip = np.zeros(nt, np.int32) if chip is None else chip
    rem, rung = C.c_double(), C.c_int()
    k = nco.nco_tail_code_ladder(1.0 / f_sf, codefreq, tc.CLEN, remcode, span, nt, NCODE, give_up, chip.ctypes.data,
                                 C.byref(rem), C.byref(rung))
    return k, rung.value, rem.value, chip[:nt]


def _random_periods(seed, count=400):
    rng = np.random.default_rng(seed)
    return [(1.023e6 + float(rng.uniform(-12, 12)), float(rng.uniform(-0.1, 1.1))) for _ in range(count)]


def test_caps_are_the_headers():
    """The tables this file counts against are the device's: GcUnitSegs, TailShared and the correlator's LDS are sized
    by them (gnsscorr_internal.h)."""
    assert (NCODE, NCAR) == (24, 40)        # (the map below was counted for these; a change moves every boundary)


@pytest.mark.parametrize("f_sf", sorted(tc.MAP), ids=lambda f: f"{f / 1e6:g}Msps")
def test_piece_count_map(nco, f_sf):
    """Pieces of the shape-specialised code step per outermost tap 1 .. 64, over 400 random periods each: the last tap
    at which every period fits GC_NCODE and the first at which none does bracket tap_span_cases.MAP.  On the far side
    the ladder with the overflow rule serves every period from the walker, in at most 20 pieces, with the chips and the
    remainder of the step; the ladder without the rule ends with an overflowed table there.  On the near side both
    serve from the step."""
    periods = _random_periods(int(f_sf) % 100003)
    lo, hi = {}, {}
    for span in range(1, 65):
        cnt = [_step_pieces(nco, f_sf, cf, rc, span) for cf, rc in periods]
        # (a period that starts behind its first wrap -- remcode >= smax ci, narrow spans only -- has no head: the step
        # declines and the walker serves, as ever)
        took = [c for c in cnt if c >= 0] or [0]
        assert len(took) >= 0.98 * len(cnt) or span * 1.023e6 / f_sf < 1.2, (span, len(took))
        lo[span], hi[span] = min(took), max(took)
    last_fit = max(s for s in range(1, 65) if all(hi[t] <= NCODE for t in range(1, s + 1)))
    first_over = min(s for s in range(1, 65) if all(lo[t] > NCODE for t in range(s, 65)))
    print(f"{f_sf / 1e6:g} Msps: every period fits up to {last_fit}, none from {first_over}; "
          f"pieces at 64: {lo[64]}..{hi[64]}")
    want_last, want_first = tc.MAP[f_sf]
    assert want_last <= last_fit < first_over <= want_first, (last_fit, first_over)
    if f_sf == 16.368e6:
        assert (lo[28], hi[28], lo[29], hi[29]) == (24, 24, 25, 25) and (last_fit, first_over) == (28, 29)
    if f_sf == 4.092e6:
        assert lo[18] > NCODE
    chip_a, chip_b = np.zeros(27000, np.int32), np.zeros(27000, np.int32)
    for span in (1, last_fit, first_over, 48, 64):
        for cf, rc in periods[:60]:
            k1, rung1, rem1, c1 = _ladder(nco, f_sf, cf, rc, span, 1, chip_a)
            k0, rung0, rem0, c0 = _ladder(nco, f_sf, cf, rc, span, 0, chip_b)
            step = _step_pieces(nco, f_sf, cf, rc, span)
            if 0 <= step <= NCODE:
                assert (k1, rung1) == (k0, rung0) == (step, 0) and rem1 == rem0 and np.array_equal(c1, c0), (span, cf, rc)
            elif step > NCODE:
                assert rung1 == 1 and 0 < k1 <= 20, (span, cf, rc, k1)
                assert k0 == -1 and rung0 == 0 and rem0 == rem1, (span, cf, rc)      # (the old ladder: served by no rung)
            else:
                assert rung1 == rung0 == 1 and k1 == k0 and 0 < k1 <= NCODE, (span, cf, rc)


@pytest.mark.parametrize("flagsync", [0, 1])
@pytest.mark.parametrize("case", tc.DEP_CASES, ids=lambda c: c["id"])
def test_state_dependent_cases_cross_the_boundary(gc, orc, nco, case, flagsync):
    """The oracle alone over the case's 40 periods per channel: in at least one channel the step needs more than
    GC_NCODE pieces in some period and at most GC_NCODE in another -- the run the device test makes changes rungs
    inside a channel, in both directions of nav-bit sync."""
    sc = tc.scene(gc, orc, case, flagsync)
    crossing = []
    for i, rows in enumerate(tc.oracle_periods(orc, sc)):
        cnt = [_step_pieces(nco, case["f_sf"], r[1], r[2], case["span"]) for r in rows]
        assert min(cnt) >= 0, (i, cnt)
        over = sum(c > NCODE for c in cnt)
        print(f"{case['id']} flagsync {flagsync} channel {i}: pieces {min(cnt)}..{max(cnt)}, {over} of {len(cnt)} over")
        crossing.append(0 < over < len(cnt))
    assert any(crossing), crossing


def test_carrier_step_has_no_such_hole(nco):
    """The carrier side of the same question: over 8000 random periods of the suite's front ends (zero IF, a quarter of
    the rate, next to Nyquist, a few Hz; phases of 0, 2 pi, next to zero, negative down to -1e6 rad) the carrier step
    never emits more pieces than the walker does on the same period -- both emit one per binade visited -- and neither
    passes GC_NCAR.  So the carrier ladder needs no overflow rule: a table the step overflows, the walker overflows."""
    rng = np.random.default_rng(40)
    idx = np.zeros(26100, np.int32)
    most_step, most_walk, took = 0, 0, 0
    for _ in range(8000):
        f_sf = float(rng.choice(sorted(tc.MAP)))
        f_if = float(rng.choice([0.0, f_sf / 4, -f_sf / 4.1, 38.4e3, f_sf * 0.4999, 1.0, 1e-3]))
        freq = f_if + float(rng.uniform(-9000, 9000)) * int(rng.integers(0, 5) > 0)
        phase = float([rng.uniform(0, DPI), 0.0, rng.uniform(0, 1) * 10.0 ** rng.uniform(-12, 1),
                       -rng.uniform(0, 1) * 10.0 ** rng.uniform(-3, 6), DPI][int(rng.integers(0, 5))])
        n = int(f_sf * 1e-3) + int(rng.integers(-2, 3))
        p = C.c_double()
        step = nco.nco_carrier_period_pieces(1.0 / f_sf, freq, phase, n, C.byref(p))
        walk = nco.nco_carrier_fast(phase, freq, 1.0 / f_sf, n, 256, idx.ctypes.data, C.byref(p))
        assert 0 < walk <= NCAR and step <= walk, (f_sf, freq, phase, n, step, walk)
        took += step > 0
        most_step, most_walk = max(most_step, step), max(most_walk, walk)
    print(f"carrier pieces: step at most {most_step} (served {took} of 8000), walker at most {most_walk}, table {NCAR}")
    assert took > 4000


def _lut(orc):
    cost, sint = np.zeros(32, np.int16), np.zeros(32, np.int16)
    orc.lib().orc_carrier_lut(cost.ctypes.data, sint.ctypes.data)
    return cost, sint


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c["id"])
def test_ladder_matches_the_literal_sequences(gc, orc, nco, case):
    """Every period of the case, before and after nav-bit sync (4 channels x 40 periods each): the sample count is the
    restated one, the code ladder's chip at every replica position and its remainder are those of the oracle's literal
    rescode() loop, the carrier ladder's LUT entry at every sample and its remainder those of mixcarr()'s, both are
    what the oracle's loop carried into the next period, and the pieces fit GC_NCODE / GC_NCAR.  Prints which rung
    served and how many pieces the carrier step took."""
    L = orc.lib()
    f_sf, span, dtype = case["f_sf"], case["span"], case["dtype"]
    ti = 1.0 / f_sf
    code = np.arange(tc.CLEN, dtype=np.int16)
    cost, sint = _lut(orc)
    ones = np.ones(case["nsamp"] + 200, np.int8)
    rungs, worst, worst_car, car_walker = [0, 0], 0, 0, 0
    for flagsync in (0, 1):
        sc = tc.scene(gc, orc, case, flagsync)
        for i, rows in enumerate(tc.oracle_periods(orc, sc)):
            for e, (carrfreq, codefreq, remcode, remcarr, n, remcode1, remcarr1) in enumerate(rows):
                where = (case["id"], flagsync, i, e)
                assert n == tc.nsamp_ref(tc.CLEN, remcode, codefreq, f_sf), where
                nt = n + 2 * span
                rc = np.zeros(nt, np.int16)
                orem = L.orc_rescode_seq(code.ctypes.data, tc.CLEN, remcode, span, ti * codefreq, n, rc.ctypes.data)
                k, rung, rem, chip = _ladder(nco, f_sf, codefreq, remcode, span, 1)
                assert 0 < k <= NCODE, where + (k,)
                assert np.array_equal(chip, rc) and rem == orem == remcode1, where
                rungs[rung] += 1
                worst = max(worst, k)
                I, Q = np.zeros(n, np.int16), np.zeros(n, np.int16)
                oprem = L.orc_mixcarr_seq(ones.ctypes.data, 1, ti, n, carrfreq, remcarr, I.ctypes.data, Q.ctypes.data)
                idx = np.zeros(n, np.int32)
                prem, crung = C.c_double(), C.c_int()
                kc = nco.nco_tail_carrier_ladder(ti, carrfreq, remcarr, n, NCAR, idx.ctypes.data, C.byref(prem), C.byref(crung))
                assert 0 < kc <= NCAR, where + (kc,)
                assert np.array_equal(cost[idx & 31], I) and np.array_equal(sint[idx & 31], Q), where
                assert prem.value == oprem == remcarr1, where
                worst_car = max(worst_car, kc)
                car_walker += crung.value
    print(f"{case['id']}: code step served {rungs[0]}, walker {rungs[1]}, at most {worst} pieces; carrier at most "
          f"{worst_car} pieces, walker {car_walker}")
    if case["dep"]:
        assert rungs[0] and rungs[1]
    elif span >= tc.MAP[f_sf][1]:
        assert rungs[0] == 0
    elif span <= tc.MAP[f_sf][0]:
        assert rungs[1] <= 2          # (a step that declines for a reason of its own: a tie, a start next to zero)
