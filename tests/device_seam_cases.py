"""The device-side seam of a GPU caller (include/gnsscorr.h: a borrowed stream, gnsscorr_trk_devptrs in stream order, a
ring filled by someone else and advanced by gnsscorr_ring_commit): the recordings, start states, feeding schedule and
the oracle's expected sums shared by tests/test_device_seam_host.py (which shows on the oracle alone that the cases can
tell an ordered reader from an unordered one) and tests/test_gpu_device_seam.py (which runs them on the device).
Helpers; not a conftest.

One instance: four GPS L1 C/A channels with the receiver's default five taps on int8 IQ samples at 4.092 Msps, zero IF,
4092 samples per code period.  A chunk is 8 code periods (32 736 samples, 65 472 bytes); the ring holds four chunks;
the stream is eight chunks, so every slot is overwritten once while the engine is live.  Two chunks are in the ring
before the first batch; batch k first writes chunk k + 2 into slot (k + 2) mod 4, commits it, and then correlates
BATCHES[k] periods with the frequencies held (gnsscorr_trk_run).  8, 8, 8 run on the look-ahead plan, 12 makes the
per-unit output buffers grow (the result pointers change), 4 reuses the larger buffers.

The reader trails the writer: batch k reads chunks k and k + 1 (of k + 1 sometimes only what its last period reaches past
the chunk's edge) and never chunk k + 2, the one written in front of it -- that is what lets a receiver write and correlate at once (the
schedule of multigpu.py).  The chunks whose writer an unordered reader would overtake are therefore the ones the batch
reads, `chunks_read`: all of them were written by the caller, the two resident ones included."""
import ctypes as C

import numpy as np

F_SF = 4.092e6
NSAMP = 4092
PERIODS_PER_CHUNK = 8
CHUNK = PERIODS_PER_CHUNK * NSAMP            # samples
CHUNK_BYTES = 2 * CHUNK
SLOTS = 4
RINGLEN = SLOTS * CHUNK                      # samples
NCHUNK = 8
RESIDENT = 2                                 # chunks in the ring before the first batch
BATCHES = (8, 8, 8, 12, 4, 8)
NTAP = 5
TAPS = dict(corrn=2, corrd=3, corrp=3)       # the receiver's default taps
CN0 = 47.0

# two instances: different satellites, different recordings (the two-thread test runs both at once)
INSTANCES = {
    "A": dict(prns=(3, 11, 19, 27), seed=5101),
    "B": dict(prns=(6, 14, 22, 31), seed=5202),
}

assert CHUNK_BYTES % 16 == 0 and sum(BATCHES) + PERIODS_PER_CHUNK <= NCHUNK * PERIODS_PER_CHUNK
assert len(BATCHES) + RESIDENT == NCHUNK


def channels(gc, inst):
    return [gc.Channel(p, dtype=2, f_sf=F_SF, f_if=0.0, **TAPS) for p in INSTANCES[inst]["prns"]]


def start_states(gc, inst):
    """Random but fixed: a carrier within the search band, a code rate within 2 Hz of nominal, remainders anywhere, the
    first period a few hundred to a few thousand samples into the stream (below one period)."""
    rng = np.random.default_rng(INSTANCES[inst]["seed"] + 1)
    crate = gc.gencode(INSTANCES[inst]["prns"][0], gc.CTYPE_L1CA)[1]
    return [dict(carrfreq=float(rng.uniform(-4000, 4000)), codefreq=crate + float(rng.uniform(-2, 2)),
                 remcode=float(rng.uniform(0.01, 0.99)), remcarr=float(rng.uniform(0, 6.2)),
                 buffloc=int(rng.integers(300, NSAMP - 300))) for _ in INSTANCES[inst]["prns"]]


_cache = {}


def stream(gc, synth, inst):
    """The recording: int8 [NCHUNK * CHUNK][2], synthesised once per process."""
    key = ("stream", inst)
    if key not in _cache:
        I = INSTANCES[inst]
        rng = np.random.default_rng(I["seed"] + 2)
        codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in I["prns"]}
        sats = [dict(prn=p, doppler=float(rng.uniform(-4000, 4000)), codephase=float(rng.uniform(0, 1023)), cn0=CN0,
                     phase=float(rng.uniform(0, 6.2))) for p in I["prns"]]
        s = synth.make_if(codes, NCHUNK * CHUNK, f_sf=F_SF, f_if=0.0, dtype=2, sats=sats, seed=I["seed"])
        s.setflags(write=False)
        _cache[key] = s
    return _cache[key]


def chunk_of(s, c):
    return s[c * CHUNK:(c + 1) * CHUNK]


def wrpos_at(k):
    """The ring's write position when batch k is issued (samples)."""
    return (RESIDENT + k + 1) * CHUNK


def stale(s, c):
    """The stream as a reader sees it that overtook the writer of chunk c: the chunk's slot still holds what it held
    before -- zeros on the first lap, the chunk four earlier afterwards."""
    t = s.copy()
    t[c * CHUNK:(c + 1) * CHUNK] = 0 if c < SLOTS else chunk_of(s, c - SLOTS)
    return t


def _chan(orc, prn, st):
    o = orc.make_chan(prn, dtype=2, f_sf=F_SF, f_if=0.0, **TAPS)
    o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
    return o


def _clone(o):
    return type(o).from_buffer_copy(o)


def _batch(orc, o, s, b, n):
    """n periods of orc_sdrtracking from sample b over the stream s (held whole, so positions are absolute): II, QQ
    [n][NTAP], sample counts [n], first samples [n], the next period's first sample."""
    ring = orc.make_ring(s, len(s), len(s) + 2 * NSAMP)      # (the write position only gates flagtrk)
    II, QQ = np.zeros((n, NTAP)), np.zeros((n, NTAP))
    ns, loc = np.zeros(n, np.int32), np.zeros(n, np.uint64)
    for e in range(n):
        orc.lib().orc_sdrtracking(C.byref(o), C.byref(ring), b)
        assert o.flagtrk
        II[e], QQ[e] = np.ctypeslib.as_array(o.II)[:NTAP], np.ctypeslib.as_array(o.QQ)[:NTAP]
        ns[e], loc[e] = o.currnsamp, b
        b += o.currnsamp
    return II, QQ, ns, loc, b


def expected(gc, orc, synth, inst):
    """The oracle's chain over the true stream: dict(batches=[per batch dict(II, QQ [nch][n][NTAP], ns, loc [nch][n])],
    state=[per channel the tracking state after the last batch], before=[per batch, per channel (oracle channel, first
    sample) as the batch starts]).  Computed once per process; treat as read-only."""
    key = ("expected", inst)
    if key in _cache:
        return _cache[key]
    s = stream(gc, synth, inst)
    prns, sts = INSTANCES[inst]["prns"], start_states(gc, inst)
    chans = [_chan(orc, p, st) for p, st in zip(prns, sts)]
    pos = [st["buffloc"] for st in sts]
    batches, before = [], []
    for n in BATCHES:
        before.append([(_clone(o), b) for o, b in zip(chans, pos)])
        rows = [_batch(orc, o, s, b, n) for o, b in zip(chans, pos)]
        pos = [r[4] for r in rows]
        batches.append(dict(II=np.stack([r[0] for r in rows]), QQ=np.stack([r[1] for r in rows]),
                            ns=np.stack([r[2] for r in rows]), loc=np.stack([r[3] for r in rows])))
        for a in batches[-1].values():
            a.setflags(write=False)
    state = [dict(carrfreq=o.carrfreq, codefreq=o.codefreq, remcode=o.remcode, remcarr=o.remcarr, buffloc=int(b))
             for o, b in zip(chans, pos)]
    _cache[key] = dict(batches=batches, state=state, before=before)
    return _cache[key]


def chunks_read(exp, k):
    """The chunks batch k reads a sample of, ascending."""
    b = exp["batches"][k]
    lo = int(b["loc"].min())
    hi = int((b["loc"].astype(np.int64) + b["ns"]).max()) - 1
    return list(range(lo // CHUNK, hi // CHUNK + 1))


def stale_batch(gc, orc, synth, inst, k, c):
    """Batch k from its true start state over stale(stream, c): (II, QQ) [nch][n][NTAP]."""
    t = stale(stream(gc, synth, inst), c)
    rows = [_batch(orc, _clone(o), t, b, BATCHES[k]) for o, b in expected(gc, orc, synth, inst)["before"][k]]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
