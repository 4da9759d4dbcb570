"""The closed loop at wide tap spans: the cases of tests/test_tap_spans_host.py (which shows on the oracle and the host
twins of gnsscorr_nco.h what each case exercises) and tests/test_gpu_tap_spans.py (which runs them on the device).
Helpers; not a conftest.

The shape-specialised code step (gc_code_period_body) spells out every replica position behind the second code wrap as
a piece of its own, about 13 + (outermost tap - samples per chip) pieces in all; the closed loop's tables hold GC_NCODE.
Where the step's pieces do not fit, the tail's table task steps down to the walker, which needs at most 20 pieces for any
span.  Whether they fit depends on the sample rate and -- at rates with a non-integer number of samples per chip -- on
the period's start phase: the rows below stand on either side of that boundary at every front end, and on it."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEN = 1023                       # every case tracks L1 C/A
NPER, NCH, CHUNKS = 40, 4, (23, 17)


def header_const(name):
    """A #define of csrc/gnsscorr_internal.h, read from the header (the cap the device uses, not a restatement)."""
    txt = open(os.path.join(ROOT, "erlangnetwork-gnsslib-sdr_amd", "csrc", "gnsscorr_internal.h")).read()
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", txt, re.M)
    assert m, name
    return int(m.group(1))


def nsamp_ref(clen, remcode, codefreq, f_sf):
    """Samples of the period that starts at code phase remcode (ref src/sdrtrk.c:31-32, as oracle/gnss_oracle.c runs it)."""
    return int((clen - remcode) / (codefreq / f_sf))


# ---- the piece-count map --------------------------------------------------------------------------------------------
# rate: (an outermost tap up to which every period's step fits GC_NCODE pieces, one from which none does), counted on
# the host over 400 random periods per span (codefreq within +-12 Hz, remcode in [-0.1, 1.1)): a bracket, which
# test_tap_spans_host.py::test_piece_count_map recounts and must land inside (DESIGN.md section 8 has its figures).
# Between the two the rung depends on the period (2.048 Msps: 14; 20 Msps: 31, 32).
MAP = {2.048e6: (13, 16), 4.092e6: (16, 18), 8.1838e6: (20, 24), 16.368e6: (28, 29), 20e6: (30, 33), 26e6: (33, 40)}

# ---- the case table -------------------------------------------------------------------------------------------------
# (corrn, corrd, corrp) per outermost tap: few taps, so that the oracle's periods stay cheap; 18 is the shipped 13-tap
# layout (CORRN 6, CORRD 3), which DESIGN.md 3.7 recorded as refused at 4.092 Msps
TAPS = {13: (1, 13, 13), 14: (2, 7, 7), 16: (2, 8, 8), 17: (1, 17, 17), 18: (6, 3, 6), 20: (4, 5, 5), 21: (3, 7, 14),
        24: (3, 8, 8), 29: (1, 29, 29), 30: (2, 15, 15), 31: (1, 31, 31), 32: (4, 8, 8), 33: (3, 11, 11), 40: (5, 8, 16),
        48: (6, 8, 8), 64: (2, 32, 32)}
TAPS64_BATCH = (16, 4, 4)         # the batched tracker's leg: 33 taps out to 64 samples

# name: front end, the spans of its row (outermost tap in samples: on either side of the rate's boundary in MAP, on it,
# and the 64 samples set_channels accepts at most), the spans at which the rung that serves depends on the period
ROWS = {
    "iq16": dict(f_sf=16.368e6, dtype=2, f_if=0.0, nsamp=16368, spans=(29, 30, 32, 33, 48, 64), dep=()),
    "iq4": dict(f_sf=4.092e6, dtype=2, f_if=0.0, nsamp=4092, spans=(18, 16, 17, 64), dep=()),
    "iq2": dict(f_sf=2.048e6, dtype=2, f_if=0.0, nsamp=2048, spans=(13, 14, 16, 64), dep=(14,)),
    "iq8": dict(f_sf=8.1838e6, dtype=2, f_if=0.0, nsamp=8183, spans=(20, 21, 24, 64), dep=()),
    "real20": dict(f_sf=20e6, dtype=1, f_if=4e6, nsamp=20000, spans=(30, 31, 32, 33, 64), dep=(31, 32)),
    "iq26": dict(f_sf=26e6, dtype=2, f_if=0.0, nsamp=26000, spans=(33, 40, 64), dep=()),
}


def _seed(row, span):
    return 7000 + 100 * sorted(ROWS).index(row) + span


# seeds of the state-dependent cases: the first of _seed + 1000 k at which, before and after nav-bit sync, a channel's
# 40 periods hold both a period whose step fits and one whose step does not (tests/test_tap_spans_host.py asserts it on
# the oracle).  k = 0 but for 31 samples at 20 Msps, where one period in 200 does not fit: k = 22, one such period in
# channel 2 of either run.
SEEDS = {("real20", 31): 7000 + 100 * 5 + 31 + 22000}

CASES = [dict(id=f"{row}_span{span}", row=row, span=span, taps=TAPS[span], seed=SEEDS.get((row, span), _seed(row, span)),
              dep=span in r["dep"], **{k: r[k] for k in ("f_sf", "dtype", "f_if", "nsamp")})
         for row, r in ROWS.items() for span in r["spans"]]
BY_ID = {c["id"]: c for c in CASES}
DEP_CASES = [c for c in CASES if c["dep"]]


def ring_samples(nsamp, nper):
    """nper periods and four more, on the ring's 16-byte granule for either sample format."""
    return -(-nsamp * (nper + 4) // 16) * 16


def scene(gc, orc, case, flagsync, taps=None, nper=NPER, nch=NCH):
    """One case's ring, channels and start states (the mix of tests/test_gpu_loop.py::_random_states_case: seeded int8
    noise; remainders of exactly 0, within 1e-6 of 0 and of 1 chip, and anywhere; Doppler up to +-9 kHz; a carrier
    phase of 0) and the oracle's channels set to them.  The same object serves the host tests and the device."""
    corrn, corrd, corrp = taps or case["taps"]
    f_sf, f_if, dtype, nsamp = case["f_sf"], case["f_if"], case["dtype"], case["nsamp"]
    rng = np.random.default_rng(case["seed"])
    nsamples = ring_samples(nsamp, nper)
    data = rng.integers(-60, 61, size=(nsamples, 2) if dtype == 2 else (nsamples,), dtype=np.int8)
    prns = [1 + (3 * i) % 32 for i in range(nch)]
    chans = [gc.Channel(p, dtype=dtype, f_if=f_if, f_sf=f_sf, corrn=corrn, corrd=corrd, corrp=corrp) for p in prns]
    states, ochs, bufflocs, nav = [], [], [], []
    for i, c in enumerate(chans):
        assert c.nsamp == nsamp and c.clen == CLEN and int(c.corrp[-1]) == corrn * corrd
        edge = i % 4
        remcode = (0.0 if edge == 0 else float(rng.uniform(0.0, 1e-6)) if edge == 1 else
                   float(1.0 - rng.uniform(0.0, 1e-6)) if edge == 2 else float(rng.uniform(0.01, 0.99)))
        st = dict(carrfreq=f_if + float(rng.uniform(-9000, 9000)), codefreq=c.crate + float(rng.uniform(-6, 6)),
                  remcode=remcode, remcarr=float(rng.uniform(0, 6.2)) if i % 5 else 0.0, buffloc=int(rng.integers(0, nsamp)))
        states.append(st)
        acqfreq = f_if + 200.0 * round((st["carrfreq"] - f_if) / 200.0)
        o = orc.make_chan(c.prn, dtype=dtype, f_sf=f_sf, f_if=f_if, corrn=corrn, corrd=corrd, corrp=corrp)
        assert o.nsamp == nsamp
        o.acq.acqfreq = acqfreq
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
        o.flagsync, o.synci, o.cnt = flagsync, (3 + 7 * i) % 20, 2001 + 3 * i
        ochs.append(o)
        bufflocs.append(C.c_uint64(st["buffloc"]))
        nav.append(dict(acqfreq=acqfreq, flagsync=flagsync, synci=o.synci, cnt=o.cnt))
    return dict(case=case, data=data, nsamples=nsamples, chans=chans, states=states, ochs=ochs, bufflocs=bufflocs, nav=nav,
                ntap=1 + 2 * corrn, smax=corrn * corrd, ring=orc.make_ring(data, nsamples, nsamples))


def oracle_periods(orc, sc, nper=NPER):
    """The oracle's closed loop alone over the scene (it consumes the scene's oracle channels): per channel, the start
    of every period -- (carrfreq, codefreq, remcode, remcarr, currnsamp) -- and the remainders it left."""
    L = orc.lib()
    out = []
    for o, b in zip(sc["ochs"], sc["bufflocs"]):
        rows = []
        for _ in range(nper):
            start = (o.carrfreq, o.codefreq, o.remcode, o.remcarr)
            assert L.orc_sdrthread_step(C.byref(o), C.byref(sc["ring"]), C.byref(b)) == 1
            rows.append(start + (o.currnsamp, o.remcode, o.remcarr))
        out.append(rows)
    return out
