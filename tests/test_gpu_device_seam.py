"""The device-side seam a GPU caller uses (-m gpu; include/gnsscorr.h): an engine on a *borrowed* stream, result
pointers in stream order (gnsscorr_trk_devptrs), a ring that someone else fills and gnsscorr_ring_commit advances.
The stream is a torch stream, the ring a torch tensor; cases and the oracle's sums come from
tests/device_seam_cases.py, and tests/test_device_seam_host.py shows on the oracle alone that a reader which overtakes
the ring's writer cannot give them.  Everything is held to bit equality; nothing here has a tolerance.

How the two sides meet.  Before a torch stream handle is given to the library the module asks the library's own HIP
runtime (through the library's handle, as tests/test_gpu_lifecycle.py reaches hipMemGetInfo) for hipStreamQuery on a torch
stream: success or not-ready shows that both sides share one runtime, any other answer fails the test by name.  Results
are captured without host synchronisation by hipMemcpyAsync, device to device, issued through the library's handle on the
borrowed stream, from the gnsscorr_trk_devptrs addresses into torch tensors (that one method, nowhere the array interface).

The delay.  Every write of ring memory stands behind a bounded delay on the stream (torch.cuda._sleep, calibrated once
with events; a chain of matmuls where that does not work), so that a reader which is not ordered behind the writer
reads the slot's old contents for certain and not by luck.  Measured on the MI355X: the host issues one steady-state
batch of scenario a (delay, copy, ring_commit, trk_run, trk_devptrs, two capture copies) in 0.07 to 0.25 ms (four runs); the
delay is DELAY_MS = 8 ms, 32 to 110 times that, and the six batches' delays with the resident chunks' one are 56 ms together
(scenario b's arm 3 has one per step, 256 ms).
"""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import device_seam_cases as dc
import lock_cases as lc
import reconfig_cases as rcases
from test_gpu_rx_lock import (verdicts, test_lock_status_equals_restatement_after_every_step,    # noqa: F401
                              test_status_history_follows_the_verdicts_and_the_schedule_rule, test_scenario_outcomes)
from test_gpu_rx_nav import lock_signal

pytestmark = pytest.mark.gpu

DELAY_MS = 8.0
HIP_SUCCESS, HIP_NOT_READY, HIP_D2D = 0, 600, 3
# Batches of scenario a after whose last call the stream must still be busy.  In batch 0 and in batch 3 (the first run,
# and the 12-period batch whose outputs grow) gnsscorr_trk_run reserves buffers and waits for the context's streams by
# itself, the caller's included: there the stream is idle by design when trk_run returns.
BUSY_BATCHES = (1, 2, 4, 5)
STEADY_BATCHES = (1, 2)         # a repeated length on the look-ahead plan: no wait of any kind inside the library

_env = {}


def _hip(gc):
    hip = gc.lib()
    hip.hipStreamQuery.argtypes = [C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return hip


def _torch(gc):
    """torch, once the library's HIP runtime has answered for a torch stream; the calibrated delay is made here too."""
    torch = pytest.importorskip("torch")
    if "rc" not in _env:
        probe = torch.cuda.Stream()
        _env["rc"] = _hip(gc).hipStreamQuery(probe.cuda_stream)
    if _env["rc"] not in (HIP_SUCCESS, HIP_NOT_READY):
        pytest.fail("torch and libgnsscorr.so do not share one HIP runtime: hipStreamQuery through the library's handle "
                    "answered %d for a torch stream; no torch stream is handed to the library" % _env["rc"])
    if "delay" not in _env:
        _env["delay"] = _make_delay(torch)
    return torch


def _make_delay(torch):
    """delay(): DELAY_MS of bounded work on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    timed(lambda: torch.cuda._sleep(1000))
    cycles = 100000
    for _ in range(4):                  # towards a probe of about the delay's length, whatever clock _sleep counts
        ms = timed(lambda: torch.cuda._sleep(cycles))
        if ms > 0.5 * DELAY_MS:
            break
        cycles = int(cycles * min(100.0, DELAY_MS / max(ms, 1e-3)))
    else:
        ms = timed(lambda: torch.cuda._sleep(cycles))
    per_ms = cycles / max(ms, 1e-3)
    if 0.5 * DELAY_MS < ms < 4 * DELAY_MS:
        n = int(per_ms * DELAY_MS)
        print("delay: torch.cuda._sleep(%d), probe %d cycles = %.3f ms" % (n, cycles, ms))
        return lambda: torch.cuda._sleep(n)
    x = torch.randn(4096, 4096, device="cuda")
    timed(lambda: x @ x)
    one = timed(lambda: x @ x)
    reps = max(1, int(np.ceil(DELAY_MS / one)))
    print("delay: %d matmuls of %.3f ms" % (reps, one))

    def chain():
        y = x
        for _ in range(reps):
            y = x @ y
    return chain


def _device_bytes(torch, a):
    """A host array as a flat int8 tensor on the device."""
    return torch.from_numpy(np.array(a, dtype=np.int8).reshape(-1)).cuda()


# ---- scenario a: the batched tracker on a borrowed stream, nothing but stream order -------------------------------------
def _scenario_a(gc, torch, synth, inst, S, nbatch=len(dc.BATCHES), barrier=None):
    """Scenario a of instance `inst` on the torch stream S: the engine borrows S, the ring is a torch tensor, every chunk
    (the two resident ones too) is copied into its slot on S behind a delay, and per batch delay, copy, ring_commit,
    trk_run, trk_devptrs and the capture copies are issued with no host synchronisation of any kind between batches.
    One synchronisation at the end.  Returns what was captured and fetched."""
    hip, delay = _hip(gc), _env["delay"]
    chans = dc.channels(gc, inst)
    nch, CB = len(chans), dc.CHUNK_BYTES
    src_t = _device_bytes(torch, dc.stream(gc, synth, inst))
    ring_t = torch.zeros(dc.SLOTS * CB, dtype=torch.int8, device="cuda")
    caps = [[torch.zeros(nch * n * dc.NTAP, dtype=torch.float64, device="cuda") for _ in range(2)] for n in dc.BATCHES[:nbatch]]
    torch.cuda.synchronize()
    out = dict(issue_ms=[], busy=[], ptrs=[])
    eng = gc.Engine(0, S.cuda_stream)
    try:
        assert eng.stream_ptr() == S.cuda_stream
        eng.ring_create(1, 2, dc.RINGLEN, ring_t.data_ptr())
        assert eng.ring_devptr(1) == ring_t.data_ptr()
        eng.set_channels(chans)
        eng.trk_set_state(dc.start_states(gc, inst))
        if barrier is not None:
            barrier.wait()
        with torch.cuda.stream(S):
            delay()
            ring_t[:dc.RESIDENT * CB].copy_(src_t[:dc.RESIDENT * CB], non_blocking=True)
        eng.ring_commit(1, dc.RESIDENT * dc.CHUNK)
        for k, n in enumerate(dc.BATCHES[:nbatch]):
            c = dc.RESIDENT + k
            slot = c % dc.SLOTS
            t0 = time.perf_counter()
            with torch.cuda.stream(S):
                delay()
                ring_t[slot * CB:(slot + 1) * CB].copy_(src_t[c * CB:(c + 1) * CB], non_blocking=True)
            eng.ring_commit(1, dc.CHUNK)
            eng.trk_run(n)
            ptrs = eng.trk_devptrs()
            for dst, p in zip(caps[k], ptrs):
                assert hip.hipMemcpyAsync(dst.data_ptr(), p, 8 * dst.numel(), HIP_D2D, S.cuda_stream) == HIP_SUCCESS
            t1 = time.perf_counter()
            out["busy"].append(not S.query())
            out["issue_ms"].append(1e3 * (t1 - t0))
            out["ptrs"].append(ptrs)
        S.synchronize()
        assert eng.ring_wrpos(1) == dc.wrpos_at(nbatch - 1)
        out["caps"] = [tuple(t.cpu().numpy().reshape(nch, n, dc.NTAP) for t in cap) for cap, n in zip(caps, dc.BATCHES)]
        out["fetch"] = eng.trk_fetch()
        out["state"] = eng.trk_get_state()
    finally:
        eng.close()
    out["ring"] = ring_t.cpu().numpy()
    return out


def _check_a(gc, orc, synth, inst, got, nbatch=len(dc.BATCHES)):
    exp = dc.expected(gc, orc, synth, inst)
    for k in range(nbatch):
        II, QQ = got["caps"][k]
        want = exp["batches"][k]
        for name, x, y in (("II", II, want["II"]), ("QQ", QQ, want["QQ"])):
            bad = np.argwhere(x != y)
            assert x.tobytes() == y.tobytes(), (inst, "batch", k, name, "%d of %d sums differ from the oracle's, first at "
                                                "(channel, period, tap) %s" % (len(bad), x.size, tuple(bad[0]) if len(bad) else "-"))
    II, QQ, ns = got["fetch"]
    assert II.tobytes() == got["caps"][nbatch - 1][0].tobytes() and QQ.tobytes() == got["caps"][nbatch - 1][1].tobytes()
    assert np.array_equal(ns, exp["batches"][nbatch - 1]["ns"])
    if nbatch == len(dc.BATCHES):
        assert got["state"] == exp["state"], (inst, got["state"], exp["state"])


def test_batched_tracker_on_a_borrowed_stream_by_stream_order_alone(gc, orc, synth):
    """Scenario a.  Six batches (8, 8, 8, 12, 4, 8 periods) with nothing but stream order between the copy that fills a
    slot, the correlator that reads it, the finish that writes the results and the copy that captures them.

    The stream must still be busy when a batch's last call has returned, or the run proved nothing: asserted for batches
    1, 2, 4 and 5.  In batches 0 and 3 gnsscorr_trk_run waits for the stream by itself (it reserves the output and plan
    buffers: first run, and the 12-period batch that makes them grow, where the result arrays are made anew); batch 5
    waits on the planner stream for the plan made for another length, which stands behind batch 4's delay, not its own.
    MI355X, four runs: the host issued batches 1 and 2 in 0.07 to 0.21 ms each (batch 0: 19 ms, batch 3: 24 ms, batch 5:
    8.2 ms, the waits named above; batch 4: up to 0.25 ms); DELAY_MS is 8 ms, 32 times the largest steady-state figure."""
    torch = _torch(gc)
    got = _scenario_a(gc, torch, synth, "A", torch.cuda.Stream())
    steady = max(got["issue_ms"][k] for k in STEADY_BATCHES)
    print("host issue time per batch (ms):", ["%.3f" % t for t in got["issue_ms"]], "steady-state", "%.3f" % steady,
          "delay", DELAY_MS, "busy after the last call:", got["busy"])
    idle = [k for k in BUSY_BATCHES if not got["busy"][k]]
    assert not idle, ("the stream was already idle when the last call of batches %s returned: this run proved nothing "
                      "about stream order (host issue %.3f ms, delay %.1f ms)" % (idle, steady, DELAY_MS))
    # the arrays are re-made at the 12-period batch (the allocator may hand out the old addresses again) and reused after it
    assert got["ptrs"][2] == got["ptrs"][1] == got["ptrs"][0] and got["ptrs"][5] == got["ptrs"][4] == got["ptrs"][3], got["ptrs"]
    _check_a(gc, orc, synth, "A", got)


# ---- scenario b: the receiver schedule, closed loop and lock monitor in three arms -------------------------------------
def _rx_arm(gc, torch, sig, sig_t, arm):
    """tests/lock_cases.py's scenario, monitor on.  arm 1: the engine's own stream, ring_push; arm 2: a borrowed stream,
    ring_push (the ingest stream's fence against a caller's stream); arm 3: a borrowed stream, the ring a torch tensor,
    every chunk copied on the stream behind a delay and committed."""
    S = torch.cuda.Stream() if arm > 1 else None
    CB = 2 * lc.CHUNK
    ring_t = torch.zeros(2 * CB, dtype=torch.int8, device="cuda") if arm == 3 else None
    torch.cuda.synchronize()
    eng = gc.Engine(0, S.cuda_stream if S is not None else None)
    try:
        eng.ring_create(1, 2, 2 * lc.CHUNK, ring_t.data_ptr() if arm == 3 else None)
        eng.set_channels(lc.channels(gc))
        eng.loop_set([eng.loop_state(i, 0.0) for i in range(len(lc.PRNS))])
        eng.rx_start(lc.RETRY_MS)
        for i, p in enumerate(lc.PRNS):
            eng.rx_lock_set(lc.prm_of(p), ch0=i, nch=1)
        hist = []
        for k in range(lc.NCHUNK):
            if arm == 3:
                slot = k % 2
                with torch.cuda.stream(S):
                    _env["delay"]()
                    ring_t[slot * CB:(slot + 1) * CB].copy_(sig_t[k * CB:(k + 1) * CB], non_blocking=True)
                eng.ring_commit(1, lc.CHUNK)
                # the chunk is not in the ring yet when the step's first launches are issued
                assert not S.query(), ("step", k, "the stream was idle before rx_step: the step proved nothing about stream order")
            else:
                eng.ring_push_raw(1, sig[k * lc.CHUNK:(k + 1) * lc.CHUNK], lc.CHUNK)
            eng.rx_step(lc.MAX_PERIODS)
            II, QQ, ns = eng.trk_fetch()
            log, ndone = eng.trk_fetch_log()
            lock, losses = eng.rx_lock_status()
            hist.append(dict(wp=eng.ring_wrpos(1), status=eng.rx_status(), I=II[:, :, 0].copy(), Q=QQ[:, :, 0].copy(), log=log,
                             ndone=ndone, lock=lock, losses=losses, II=II, QQ=QQ, ns=ns))
        return hist
    finally:
        eng.close()


def _arm(gc, synth, arm):
    torch = _torch(gc)
    sig = lock_signal(gc, synth)
    if arm == 3 and "sig_t" not in _env:
        _env["sig_t"] = _device_bytes(torch, sig)
    return _rx_arm(gc, torch, sig, _env.get("sig_t"), arm)


@pytest.fixture(scope="module")
def arm1(gc, synth):
    return _arm(gc, synth, 1)


@pytest.fixture(scope="module")
def arm2(gc, synth):
    return _arm(gc, synth, 2)


@pytest.fixture(scope="module")
def arm3(gc, synth):
    try:
        return _arm(gc, synth, 3)
    finally:
        _env.pop("sig_t", None)         # 65 MB of device memory


@pytest.fixture(scope="module")
def runs(arm1):
    """Arm 1 as tests/test_gpu_rx_lock.py's `runs`: its checks, imported above, run on it in this module."""
    return dict(on=arm1)


def _same_steps(a, b, what):
    """Every step's log, ndone, II, QQ, sample counts, rx_status, rx_lock_status and losses, byte for byte."""
    assert len(a) == len(b) == lc.NCHUNK and [h["wp"] for h in a] == lc.step_wrpos()
    assert any(np.any(h["ndone"] > 0) for h in a) and any(np.any(h["losses"]) for h in a)      # not an idle receiver
    for k, (x, y) in enumerate(zip(a, b)):
        rcases.same(x, y, (what, "step", k))


def test_receiver_schedule_on_a_borrowed_stream_fed_by_ring_push_equals_own_stream(arm1, arm2):
    """Arm 2 against arm 1: the ingest stream's fence against a caller's stream."""
    _same_steps(arm1, arm2, "borrowed stream, ring_push")


def test_receiver_schedule_on_a_borrowed_stream_and_committed_ring_equals_own_stream(arm1, arm3):
    """Arm 3 against arm 1.  Its first launches of a step -- the search of the due channels, the closed loop -- read the
    chunk just written on the stream; without stream order they would read the chunk of two steps before."""
    _same_steps(arm1, arm3, "borrowed stream, committed ring")


# ---- scenario c: two engines, two threads ------------------------------------------------------------------------------
def test_two_engines_from_two_threads_on_two_streams(gc, orc, synth):
    """Two instances of scenario a -- other satellites, other recordings -- on two torch streams from two host threads
    that start together at a barrier; the library's process-wide state (the correlator form chosen lazily, the kernels'
    attributes) is first touched by both at once.  Each must equal its oracle."""
    torch = _torch(gc)
    for inst in ("A", "B"):                 # host-side inputs once, outside the threads
        dc.stream(gc, synth, inst)
    barrier = threading.Barrier(2)
    streams = {inst: torch.cuda.Stream() for inst in ("A", "B")}
    got, err = {}, {}

    def work(inst):
        try:
            got[inst] = _scenario_a(gc, torch, synth, inst, streams[inst], barrier=barrier)
        except BaseException as e:           # noqa: B036 (reported in the main thread)
            err[inst] = e
            barrier.abort()

    threads = [threading.Thread(target=work, args=(inst,)) for inst in ("A", "B")]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not err, err
    for inst in ("A", "B"):
        _check_a(gc, orc, synth, inst, got[inst])


# ---- scenario d: the lifecycle of what is borrowed ----------------------------------------------------------------------
def test_lifecycle_of_a_borrowed_stream_and_ring(gc, orc, synth):
    torch = _torch(gc)
    L = gc.lib()
    S = torch.cuda.Stream()
    # torch's default stream has the null handle: it cannot be borrowed, the engine answers it with a stream of its own
    assert torch.cuda.default_stream().cuda_stream == 0
    own = [gc.Engine(0), gc.Engine(0, torch.cuda.default_stream().cuda_stream)]
    try:
        assert own[0].stream_ptr() and own[1].stream_ptr() and own[0].stream_ptr() != own[1].stream_ptr()
        assert S.cuda_stream not in (own[0].stream_ptr(), own[1].stream_ptr())
    finally:
        for e in own:
            e.close()
    eng = gc.Engine(0, S.cuda_stream)
    try:
        assert eng.stream_ptr() == S.cuda_stream                    # the handle that was given
        eng.ring_create(1, 2, dc.RINGLEN)
        eng.set_channels(dc.channels(gc, "A"))
        a, b = C.c_void_p(), C.c_void_p()
        assert L.gnsscorr_trk_devptrs(eng.h, C.byref(a), C.byref(b)) == gc.ESTATE and a.value is None and b.value is None
        with pytest.raises(gc.GnsscorrError, match="trk_devptrs"):
            eng.trk_devptrs()
        # gnsscorr_sync on a borrowed stream returns once the caller's stream is idle
        with torch.cuda.stream(S):
            _env["delay"]()
        assert not S.query(), "the delay was over before gnsscorr_sync was called: nothing shown"
        eng.sync()
        assert S.query()
    finally:
        eng.close()
    # batch 0 of scenario a on S, and again on the same S with a second engine after the first was closed
    first = _scenario_a(gc, torch, synth, "A", S, nbatch=1)
    with torch.cuda.stream(S):                                      # S outlives the engine: it accepts work and synchronises
        x = torch.arange(1000, device="cuda", dtype=torch.float64).sum()
    S.synchronize()
    assert float(x) == 499500.0 and S.query()
    second = _scenario_a(gc, torch, synth, "A", S, nbatch=1)
    for got in (first, second):
        _check_a(gc, orc, synth, "A", got, nbatch=1)
        # close() left the caller's ring tensor alone: three chunks as written, the fourth slot untouched
        want = np.zeros(dc.SLOTS * dc.CHUNK_BYTES, np.int8)
        want[:3 * dc.CHUNK_BYTES] = dc.stream(gc, synth, "A").reshape(-1)[:3 * dc.CHUNK_BYTES]
        assert got["ring"].tobytes() == want.tobytes()
