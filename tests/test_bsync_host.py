"""Bit synchronisation by symbol energy on the CPU oracle and the restatement alone (no GPU): the identities the rules
rest on, what the reference's checksync() does with the scenario of tests/bsync_cases.py (the control), what the detector
(tests/bsync_restate.py) decides over the same rows and with how much room, the bits decided behind a preset, and the
same at rate 2 for PRN 133 of tests/lock_sbas_cases.py.  The numbers asserted here were measured here; DESIGN.md 3.2g
carries them as tables."""
import numpy as np
import pytest

import bsync_cases as bc
import bsync_restate as br
import lock_cases as lc
import lock_sbas_cases as ls

WATCH = dict(bc.PRM, gate=1e9, nsym_max=4096)       # the detector watching only: every test's ratio, no decision


# ---- identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", range(2, 21))
def test_every_offset_has_exactly_n_whole_symbols_at_a_test(R):
    """Rule 7: at the rows with (L + 1) mod R == 0 every offset has completed exactly n = (L + 1)/R - 1 symbols, and
    at no other row do all offsets agree -- for every a0 mod R, fed row by row (the state does not depend on the cut).
    Constant prompts of 1: a whole symbol adds R*R to its offset's E."""
    prm = dict(start_cnt=0, nsym=1, nsym_max=4096, gate=1e9)
    for a0 in range(3 * R, 4 * R):
        st = br.zero_state()
        for c in range(a0, a0 + 6 * R):
            br.run(st, prm, R, [1.0], [0.0], [0], 1, c)
            L = c - a0 + 1
            # counted directly: symbols of offset o start at s = o (mod R), s >= a0, and are whole when s + R - 1 <= c
            whole = [len([s for s in range(a0, c + 1) if s % R == o and s + R - 1 <= c]) for o in range(R)]
            assert [e / (R * R) for e in st["E"][:R]] == whole, (R, a0, c)
            if (L + 1) % R == 0:
                assert whole == [(L + 1) // R - 1] * R and st["n"] == whole[0], (R, a0, c, whole)
            elif L + 1 > R:
                assert len(set(whole)) == 2, (R, a0, c, whole)
        assert st["armed"] == 1 and st["a0"] == a0 and st["tests"] == 5


@pytest.mark.parametrize("R", [2, 3, 7, 10, 20])
def test_noiseless_prompts_give_the_layouts_synci(R):
    """Symbols tied to the code as synth.make_if lays them out, no noise: for every alignment of row 0 in its symbol and
    every start of the span the detector decides at its first test, on the layout's synci."""
    rng = np.random.default_rng(R)
    sym = rng.choice([-1.0, 1.0], size=400)
    sym[:40:2], sym[1:40:2] = 1.0, -1.0                             # (transitions inside any span of a few symbols)
    for p0 in range(R):
        for cnt0, start in ((0, 0), (137, 140), (4001, 4001 + R // 2)):
            n = 12 * R
            I = np.array([700.0 * sym[(p0 + e) // R] for e in range(n)])
            Q = np.array([-300.0 * sym[(p0 + e) // R] for e in range(n)])
            st, ev = br.zero_state(), []
            br.run(st, dict(start_cnt=start, nsym=8, nsym_max=8, gate=1.5), R, I, Q, np.zeros(n, int), n, cnt0, events=ev)
            want = br.layout_synci(p0, cnt0, R)
            assert (st["done"], st["synci"], st["tests"]) == (1, want, 1), (R, p0, cnt0, st)
            assert st["best"] == (want + 1) % R and st["decided_cnt"] == max(start, cnt0) + 9 * R - 2


def test_layout_synci_is_sync_if_cases_synci():
    import sync_if_cases as sic
    assert [br.layout_synci(sic.p0(i), sic.CNT0[i], 20) for i in range(3)] == [sic.synci(i) for i in range(3)]


# ---- the scenario on the oracle ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sig(gc, synth):
    return bc.signal(gc, synth)


@pytest.fixture(scope="module")
def control(gc, orc, sig):
    """The reference's rule alone: A, B, C."""
    return [bc.oracle_run(gc, orc, sig, i) for i in range(3)]


@pytest.fixture(scope="module")
def detected(gc, orc, sig):
    """The detector with the chosen parameters and the poke at the next step boundary: A, B, C."""
    return [bc.oracle_run(gc, orc, sig, i, prm=bc.PRM) for i in range(3)]


def _agreement(i, rows, from_cnt=0):
    """(decided bits from from_cnt on, those equal to the bit sent)."""
    j = np.flatnonzero((rows["navbit"] != 0) & (rows["cnt"] >= from_cnt))
    sent = bc.sent_bits(i, bc.P0[i], rows["cnt"][j])
    return len(j), int(np.sum(rows["navbit"][j] == np.array(sent)))


def test_control_reference_rule_on_the_oracle(control):
    """What checksync() does with the scenario: A synchronises at cnt 2020 with synci 0, ten periods off the true edge;
    B at cnt 2030 on the true edge; C (the vote branch) not within the 3 s."""
    p0 = [bc.code_period(i, r["handover"]) for i, r in enumerate(control)]
    assert tuple(p0) == bc.P0 and [p % 20 for p in p0] == [9, 9, 9]
    truth = [bc.true_synci(i) for i in range(3)]
    print("reference rule: (cnt, synci) %s, true synci %s" % ([r["sync"] for r in control], truth))
    assert truth == [10, 10, 10]
    assert control[0]["sync"] == (2020, 0)                          # wrong: wherever the true edge is
    assert control[1]["sync"] == (2030, 10)
    assert control[2]["sync"] is None and len(control[2]["rows"]["cnt"]) > 2700
    # the bits sent around A's periods 2001 .. 2020 are alike, B's are not
    for i, alike in ((0, True), (1, False)):
        b = bc.bits(i)
        s = (bc.P0[i] + 2001) // 20
        assert (bc.P0[i] + 2020) // 20 == s + 1 and (b[s] == b[s + 1]) == alike


def test_detector_on_the_oracle_with_room(gc, orc, sig, detected):
    """The decision of A, B and C: at the first test (25 bits from cnt 200: cnt 718), on the true edge, the deciding
    ratio far above the gate; the tracker on noise (the absent PRN, handed over by force) never comes near it."""
    noise = bc.oracle_run(gc, orc, sig, 3, prm=WATCH, force=True)
    nr = [e[4] for e in noise["events"]]
    deciding = []
    for i, r in enumerate(detected):
        st = r["st"]
        print("%s: decided at cnt %d, synci %d, ratio %.1f" % (bc.NAMES[i], st["decided_cnt"], st["synci"], st["ratio_last"]))
        assert (st["done"], st["synci"], st["decided_cnt"], st["tests"]) == (1, bc.true_synci(i), 718, 1), (i, st)
        assert st["best"] == 11 and st["a0"] == bc.START_CNT
        deciding.append(st["ratio_last"])
    print("noise: ratios at %s: %s" % ([e[2] for e in noise["events"]], ["%.2f" % x for x in nr]))
    assert len(nr) >= 5 and noise["sync"] is None
    # the room: chosen from these measurements (bsync_cases.PRM), 10 % on either side of the gate at the least
    assert min(deciding) >= 1.1 * bc.GATE and max(nr) <= 0.9 * bc.GATE
    # the measured figures, to the digits given
    assert [round(x) for x in deciding] == [1431, 750, 469]
    assert max(nr) == nr[0] and round(nr[0], 2) == 1.55
    # with the chosen parameters the noise channel is given up at nsym_max and left to the reference's rule
    given_up = bc.oracle_run(gc, orc, sig, 3, prm=bc.PRM, force=True)
    assert (given_up["st"]["done"], given_up["st"]["n"], given_up["st"]["tests"], given_up["poked"]) == (2, 100, 4, None)


def test_bits_after_the_preset_and_under_the_reference_rule(control, detected):
    """The poke at the step boundary behind the decision (step 4, cnt 760): from there to the end every decided bit is
    the bit sent, up to one polarity, for A, B and C.  Under the reference's own rule A's bits are not: it integrates
    half of one bit and half of the next."""
    for i, r in enumerate(detected):
        assert r["poked"] == 4 and r["sync"] == (760, bc.true_synci(i))
        n, ok = _agreement(i, r["rows"])
        assert n == 100 and ok in (0, n), (i, n, ok)
    n, ok = _agreement(0, control[0]["rows"])
    print("A under the reference's rule: %d of %d decided bits equal the bits sent" % (ok, n))
    assert n == 37 and 0.25 * n < ok < 0.75 * n
    n, ok = _agreement(1, control[1]["rows"])
    assert n == 37 and ok in (0, n)                                 # B: the right edge, late


# ---- SBAS, rate 2 -----------------------------------------------------------------------------------------------------
SBAS_PRM = bc.SBAS_PRM


def test_sbas_prn133_decides_the_right_edge_before_cnt_2000(gc, orc, synth):
    """PRN 133 of tests/lock_sbas_cases.py, whose first hand-over the reference's rule synchronises at cnt 2002 on the
    wrong symbol edge: the detector decides the right one at cnt 400.  The first three generator chunks of that signal
    (3 * 2^22 samples, identical to the start of the whole recording) hold all that is needed.  Random symbols: about
    half have a transition, so the ratio is just below 2, against 1.0 .. 1.13 on noise."""
    n = 3 << 22
    codes = {p: gc.gencode(p, ct) for p, ct, _, _, _ in ls.CHANNELS}
    codes[122] = gc.gencode(122, lc.CTYPE_SBAS)
    sig = synth.make_if(codes, n, f_sf=ls.F_SF, f_if=0.0, dtype=2, sats=ls.sats(), seed=ls.SEED)
    wr = [w for w in ls.step_wrpos() if w <= n]
    chan = lambda prn: dict(prn=prn, ctype=lc.CTYPE_SBAS, f_sf=ls.F_SF, nsamp=ls.NSAMP, rate=2, taps=ls.TAPS, first_try=lc.FIRST_TRY)
    run = lambda prn, prm, **kw: bc.oracle_run(gc, orc, sig, 1, prm=prm, wrpos=wr, max_periods=ls.MAX_PERIODS, chan=chan(prn), **kw)
    ref = run(133, None)
    row, synci, right, _ = ls.predict(1, ref["handover"])
    truth = br.layout_synci(ls.code_period(1, ref["handover"]), 0, 2)
    assert ref["sync"] == (row, synci) == (2002, 0) and not right and truth == 1
    watch = run(133, dict(SBAS_PRM, gate=1e9, nsym_max=4096))
    ratios = [e[4] for e in watch["events"]]
    assert len(ratios) >= 8 and all(e[3] == 0 for e in watch["events"])
    noise = run(122, dict(SBAS_PRM, gate=1e9, nsym_max=4096), force=True)
    nr = [e[4] for e in noise["events"]]
    print("PRN 133: ratios %s; noise: %s" % (["%.2f" % x for x in ratios], ["%.2f" % x for x in nr]))
    assert min(ratios) >= 1.1 * SBAS_PRM["gate"] and len(nr) >= 8 and max(nr) <= 0.9 * SBAS_PRM["gate"]
    assert round(min(ratios), 2) == 1.75 and max(nr) < 1.10
    got = run(133, SBAS_PRM)
    st = got["st"]
    assert (st["done"], st["synci"], st["decided_cnt"], st["tests"]) == (1, truth, 400, 1), st
    assert got["sync"] is not None and got["sync"][1] == truth and got["sync"][0] < 2000
    # every symbol decided from the preset on is the symbol sent, up to one polarity
    rows, p = got["rows"], ls.code_period(1, got["handover"])
    j = np.flatnonzero(rows["navbit"])
    sent = ls.symbols()[(p + rows["cnt"][j]) // 2]
    ok = int(np.sum(rows["navbit"][j] == sent))
    assert len(j) > 1000 and ok in (0, len(j)), (len(j), ok)
