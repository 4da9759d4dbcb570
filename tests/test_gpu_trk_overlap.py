"""The batched tracker with its table kernels beside the previous batch's correlator (gnsscorr_trk.hip, correlate_slot;
DESIGN 3.1): trk_expand, trk_ringcheck and trk_edges of batch k+1 are queued on a stream of their own and may run while
the correlator of batch k runs, each plan slot has its own edge table, trk_finish follows its correlator on the main
stream, and the planner chain waits for nothing of a slot but the tables that read its plan entries.

Batches issued back to back, with no fetch or synchronisation in between, must leave what an engine leaves that waits
for every batch before it issues the next: the last batch's per-period outputs, sample counts and sums, and the state,
byte for byte.  Two runs of the same kernels on the same samples: no tolerance anywhere."""
import struct

import numpy as np
import pytest

from test_gpu_lifecycle import NSAMP, _states

pytestmark = pytest.mark.gpu
ESTATE = -3
PERIODS = 5 * 130 + 6              # the longest sequence below, past the channels' start positions (100 + 900 i samples)

PATTERNS = {
    "65": lambda k: [65] * k,                    # every batch after the first on the look-ahead plan, both slots in turn
    "1": lambda k: [1] * k,                      # one period: tables of a single partial workgroup
    "130": lambda k: [130] * k,
    "4/7": lambda k: [4, 7, 4, 7, 4][:k],        # the plan made ahead is dropped every time; the buffers grow at the 7
    "7/4": lambda k: [7, 4, 7, 4, 7][:k],        # ... and the shorter second batch runs in buffers that do not grow
}


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(53).integers(-60, 61, size=(NSAMP * PERIODS, 2), dtype=np.int8)


@pytest.fixture(scope="module")
def chans(gc):
    return [gc.Channel(p, dtype=2, f_if=0.0) for p in (2, 7, 12, 19, 30)]


def _engine(gc, data, chans, poison, pushed=None):
    e = gc.Engine(0)
    if poison is not None:
        e.debug_poison(poison)         # every buffer made from here on starts as 0xA5 bytes, not as zeros
    e.ring_create(1, 2, data.shape[0])
    n = data.shape[0] if pushed is None else pushed
    e.ring_push_raw(1, data[:n], n)
    e.set_channels(chans)
    return e


def _bits(states):
    return [struct.pack("<ddddQ", s["carrfreq"], s["codefreq"], s["remcode"], s["remcarr"], s["buffloc"]) for s in states]


def _run(gc, data, chans, poison, lengths, sync_each):
    eng = _engine(gc, data, chans, poison)
    try:
        eng.trk_set_state(_states(chans, 61))
        for n in lengths:
            eng.trk_run(n)
            if sync_each:
                eng.sync()
        sums = eng.trk_fetch_sums()
        II, QQ, ns = eng.trk_fetch()
        return [sums[0], sums[1], II, QQ, ns], _bits(eng.trk_get_state())
    finally:
        eng.close()


@pytest.mark.parametrize("poison", [None, 0xA5], ids=["plain", "poisoned"])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_back_to_back_batches_equal_synchronised_ones(gc, noise, chans, pattern, poison):
    """5 channels of the 5-tap default, K = 1..5 batches.  On the poisoned engine a correlator that read the other
    slot's edge table, or a table not yet written, would read 0xA5A5 start samples where the reference engine (its
    batches serialised by sync()) reads the slot's own."""
    for k in range(1, 6):
        lengths = PATTERNS[pattern](k)
        a, sa = _run(gc, noise, chans, poison, lengths, sync_each=False)
        b, sb = _run(gc, noise, chans, poison, lengths, sync_each=True)
        for i, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (pattern, k, i)
        assert sa == sb, (pattern, k)
        assert a[4].min() > 0 and np.abs(a[2]).max() > 0, (pattern, k)          # something was correlated
        assert int(a[4].sum()) > 0


def test_poisoned_and_plain_engines_agree(gc, noise, chans):
    """What a batch leaves does not depend on what its buffers held before: three batches of 65 on a plain and on a
    poisoned engine."""
    a, sa = _run(gc, noise, chans, None, [65] * 3, sync_each=False)
    b, sb = _run(gc, noise, chans, 0xA5, [65] * 3, sync_each=False)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), i
    assert sa == sb


@pytest.mark.parametrize("sync_each", [False, True], ids=["back_to_back", "synchronised"])
def test_ring_violation_is_reported_by_the_fetch(gc, noise, chans, sync_each):
    """The ring holds 100 periods; three batches of 65 are planned, so the second batch runs past the write position.
    The ring check counts on the tables stream: the fetch behind the third batch must still answer
    GNSSCORR_ESTATE, and the fetch after it (the counter read and cleared) succeeds."""
    L = gc.lib()
    eng = _engine(gc, noise, chans, None, pushed=100 * NSAMP)
    try:
        eng.trk_set_state(_states(chans, 61))
        for _ in range(3):
            eng.trk_run(65)
            if sync_each:
                eng.sync()
        II, QQ = np.zeros((5, 65, 5)), np.zeros((5, 65, 5))
        ns = np.zeros((5, 65), np.int32)
        assert L.gnsscorr_trk_fetch(eng.h, II.ctypes.data, QQ.ctypes.data, ns.ctypes.data) == ESTATE
        assert "outside what the IF ring holds" in L.gnsscorr_last_error().decode()
        assert L.gnsscorr_trk_fetch(eng.h, II.ctypes.data, QQ.ctypes.data, ns.ctypes.data) == 0
    finally:
        eng.close()
