"""What the schedule's three stages behind the closed loop share (-m gpu): the lock monitor, bit
synchronisation by symbol energy and the correlation monitor go through one stage record, one staging path and one rows
view, so the properties below are asked of all three alike.

Bars, all exact: a state that no gnsscorr_rx_*_set has named reads as zero bytes, on an engine whose device buffers are
poisoned before first use; a channel range that overflows an int is refused; gnsscorr_rx_start leaves every stage off
and every state, count and loss zero; and a *_run through the shared staging buffer returns the bytes the same call
returns on a fresh engine, whatever ran through the buffer before, and equals the host restatement."""
import numpy as np
import pytest

import bsync_cases as bc
import cfm_cases as cc
import lock_cases as lc
import lock_restate as lr
import test_gpu_bsync as tb
import test_gpu_cfm as tc
import test_gpu_lock as tl

pytestmark = pytest.mark.gpu
NCH = len(bc.PRNS)
A, B, CC = 0, 1, 2
CFM_PRM = cc.prm(npair=1)


def _schedule(gc, poison=None):
    """An engine with the four channels of tests/bsync_cases.py and a schedule started, no sample pushed."""
    eng = gc.Engine(0)
    try:
        if poison is not None:
            eng.debug_poison(poison)
        eng.ring_create(1, 2, 2 * bc.CHUNK)
        eng.set_channels(bc.channels(gc))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(NCH)])
        eng.rx_start(bc.RETRY_MS)
    except Exception:
        eng.close()
        raise
    return eng


def _stages(eng):
    """(name, set, states, parameters) of the three stages."""
    return (("lock", eng.rx_lock_set, lambda: eng.rx_lock_status()[0], lc.PRM),
            ("bsync", eng.rx_bsync_set, lambda: eng.rx_bsync_status()[0], bc.PRM),
            ("cfm", eng.rx_cfm_set, eng.rx_cfm_status, CFM_PRM))


def _zero(a):
    return a.tobytes() == bytes(a.nbytes)


def test_channels_never_named_read_zero_on_a_poisoned_engine(gc):
    """The first set of each stage names channel 1 alone: channel 1 is freshly zeroed, the others were never written by
    any call, and the state buffer was made full of 0xA5."""
    eng = _schedule(gc, poison=0xA5)
    try:
        for name, set_, states, prm in _stages(eng):
            set_(prm, ch0=1, nch=1)
            st = states()
            assert st.shape == (NCH,)
            for i in range(NCH):
                assert _zero(st[i]), (name, i)
        assert not np.any(eng.rx_bsync_status()[1]) and not np.any(eng.rx_lock_status()[1])
    finally:
        eng.close()


def test_a_channel_range_that_overflows_is_refused(gc):
    eng = _schedule(gc, poison=0xA5)
    try:
        for name, set_, states, prm in _stages(eng):
            with pytest.raises(gc.GnsscorrError, match="channels"):
                set_(prm, ch0=1, nch=2 ** 31 - 1)
            assert _zero(states()), name
        assert not np.any(eng.rx_bsync_status()[1]) and not np.any(eng.rx_lock_status()[1])
    finally:
        eng.close()


def test_rx_start_starts_every_stage_over(gc, synth):
    """The scenario of tests/bsync_cases.py with all three stages on.  A's lock monitor has a time limit it cannot meet,
    so A is sent back to SEARCH; B and C are preset behind the fourth step, so the fifth step's rows are synchronised and
    reach the lock monitor's sums.  Then gnsscorr_rx_start: everything reads zero and the next step launches no stage."""
    sig = bc.signal(gc, synth)
    eng = _schedule(gc)
    try:
        eng.timing(True)
        eng.rx_lock_set(lc.PRM)
        eng.rx_lock_set(dict(lc.PRM, sync_periods=300), ch0=A, nch=1)
        eng.rx_bsync_set(bc.PRM)
        eng.rx_cfm_set(CFM_PRM)

        def step(k):
            eng.ring_push_raw(1, sig[k * bc.CHUNK:(k + 1) * bc.CHUNK], bc.CHUNK)
            eng.rx_step(bc.MAX_PERIODS)

        for k in range(5):
            step(k)
        lock, losses = eng.rx_lock_status()
        bsync, applied = eng.rx_bsync_status()
        assert not _zero(lock[CC]) and lock[CC]["open"] == 1 and losses[A] >= 1
        assert bsync[CC]["done"] == 1 and applied[CC] == 1
        names = ("rx_lock", "rx_bsync", "rx_cfm")
        launches = [eng.timing_read(n)[1] for n in names]
        assert launches == [5, 5, 5]
        eng.rx_start(bc.RETRY_MS)
        lock, losses = eng.rx_lock_status()
        bsync, applied = eng.rx_bsync_status()
        assert _zero(lock) and _zero(bsync) and _zero(eng.rx_cfm_status())
        assert not np.any(losses) and not np.any(applied)
        step(5)
        assert [eng.timing_read(n)[1] for n in names] == launches
        assert _zero(eng.rx_lock_status()[0]) and _zero(eng.rx_bsync_status()[0]) and _zero(eng.rx_cfm_status())
    finally:
        eng.close()


def _cut(case, rates, nch, nper):
    """The first nch channels and nper rows of a generated case of any of the three kinds, and their rates."""
    prm, I, Q, log, ndone, cnt0, st = case
    return (prm[:nch], np.ascontiguousarray(I[:nch, :nper]), np.ascontiguousarray(Q[:nch, :nper]),
            np.ascontiguousarray(log[:nch, :nper]), np.minimum(ndone[:nch], nper).astype(np.int32), cnt0[:nch], st[:nch]), rates[:nch]


def _calls(gc, big_first):
    """lock_run, cfm_run (corrn 16), bsync_run, cfm_run (corrn 1), lock_run on the inputs of tests/test_gpu_lock.py,
    test_gpu_bsync.py and test_gpu_cfm.py, 5 channels x 65 rows (a workgroup of four wavefronts and one of one; a second
    chunk of one row) alternating with 1 x 1: per call what runs it on an engine, and what checks it against the
    restatement."""
    big, small = (5, 65), (1, 1)
    shapes = [big if (k % 2 == 0) == big_first else small for k in range(5)]

    def lock(k, seed):
        case, rates = _cut(tl._case(gc, 65, "five", seed), tl.RATES, *shapes[k])

        def check(got):
            want = tl._restate(*case, rates=rates)
            for i, w in enumerate(want):
                assert lr.same(w, got[i]) == [], ("lock", k, i)
        return (lambda eng: tl._device(gc, eng, *case, rates=rates)), check

    def bsync(k, seed):
        case, rates = _cut(tb._case(gc, 65, "early", seed), tb.RATES, *shapes[k])
        return (lambda eng: tb._device(gc, eng, *case, rates=rates)), (lambda got: tb._assert_same(tb._restate(*case, rates=rates), got))

    def cfm(k, corrn, seed):
        case, rates = _cut(tc._case(gc, corrn, seed), tc.RATES, *shapes[k])
        return ((lambda eng: tc._device(gc, eng, corrn, *case, rates=rates)),
                (lambda got: tc._assert_same(tc._restate(corrn, *case, rates=rates), got)))

    return [lock(0, 11), cfm(1, 16, 12), bsync(2, 13), cfm(3, 1, 14), lock(4, 15)]


@pytest.mark.parametrize("big_first", [True, False])
def test_the_staging_buffer_is_shared_across_stages_and_sizes(gc, big_first):
    calls = _calls(gc, big_first)
    shared = gc.Engine(0)
    try:
        for k, (run, check) in enumerate(calls):
            got = run(shared)
            fresh = gc.Engine(0)
            try:
                alone = run(fresh)
            finally:
                fresh.close()
            assert got.tobytes() == alone.tobytes(), k
            check(got)
    finally:
        shared.close()
