"""SBAS L1 frame synchronisation on the GPU (-m gpu): gnsscorr_sbasframe_replay (Viterbi decodes on the device, the
walk on the host) against the plain Python replay of fec_restate.py, field for field, on synthetic closed-loop logs --
rows that carry only navbit and buffloc.  The streams and what the replay must find in them are those test_fec_host.py
holds the restatement itself to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fec_restate as fr  # noqa: E402
import sbas_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["pol+1_lead0", "pol+1_lead7", "pol-1_lead0", "pol-1_lead7", "flagpol", "noframe", "aid", "noaid"]


def _log(gc, navbit, buffloc):
    log = np.zeros(len(navbit), dtype=np.dtype(gc.TrkLog))
    log["navbit"] = navbit
    log["buffloc"] = buffloc
    return log


def _fields(st):
    return {f: getattr(st, f) for f in fr.FIELDS} | {"msg": bytes(st.msg)}


def _same(st, rep):
    assert _fields(st) == rep.fields()
    assert st.tow == rep.tow
    assert np.array_equal(np.ctypeslib.as_array(st.fbits), rep.fbits)


@pytest.mark.parametrize("name", NAMES)
def test_replay_equals_the_restatement(gc, engine, name):
    case, rep, (navbit, buffloc, cnts, locs, aid) = sc.replayed(name)
    st = gc.SbasFrameState()
    engine.sbasframe_replay(st, _log(gc, navbit, buffloc), 0, aid, sc.AID_WEEK if case["aid"] else 0)
    _same(st, rep)
    # and what the restatement found is what the stream was built to hold (test_fec_host.py)
    assert st.flagpol == case["flagpol"]
    if case["found"] is None:
        assert st.flagtow == 0 and st.flagdec == 0
    else:
        assert st.flagdec == 1 and st.firstsfcnt == cnts[case["found"]] and st.polarity == case["polarity"]


@pytest.mark.parametrize("name,cnt0", [("pol-1_lead7", 0), ("flagpol", 123456789), ("aid", 4000)])
def test_replay_in_pieces_of_97_periods(gc, engine, name, cnt0):
    case, rep, (navbit, buffloc, cnts, locs, aid) = sc.replayed(name, first_period=5, cnt0=cnt0)
    log = _log(gc, navbit, buffloc)
    st = gc.SbasFrameState()
    for i in range(0, len(log), 97):
        engine.sbasframe_replay(st, log[i:i + 97], cnt0 + i, None if aid is None else aid[i:i + 97],
                                sc.AID_WEEK if case["aid"] else 0)
    _same(st, rep)
    assert st.firstsfcnt == cnt0 + 5 + 2 * case["found"]


def test_bad_arguments(gc, engine):
    st = gc.SbasFrameState()
    log = _log(gc, np.ones(4, np.int32), np.zeros(4, np.uint64))
    assert gc.lib().gnsscorr_sbasframe_replay(None, st, log.ctypes.data, 4, 0, None, 0) == -1    # no context: no CPU path
    assert gc.lib().gnsscorr_sbasframe_replay(engine.h, st, log.ctypes.data, -1, 0, None, 0) == -1
    engine.sbasframe_replay(st, _log(gc, np.zeros(10, np.int32), np.zeros(10, np.uint64)))      # no symbol: no work
    assert _fields(st) == fr.SbasReplay().fields()
