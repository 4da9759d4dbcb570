"""Scenarios of the mixed-receiver schedule tests (tests/test_rx_mixed_host.py shows on the oracle alone that they
decide what they claim, tests/test_gpu_rx_mixed.py runs them on the device; not a conftest).

MIX -- the schedule on two rings, shaped like BASELINE configs[3]:
  ring 1, int8 IQ at 16.368 Msps: L1 C/A present / absent / rising late, SBAS, and one L1 C/A channel with intg 3 on
  a 500 Hz grid whose first try comes after 4 code periods instead of 11;
  ring 2, real samples at 20 Msps on a 4 MHz IF (the 65536-point transform): L1 C/A present / absent, GLONASS G1
  present / rising late.
Step k pushes ring 1 (6 code periods at k = 0, 0.1 s afterwards) and, from step 3 on and not in steps 6 and 9,
0.08 s of ring 2; then one gnsscorr_rx_step.  A failed search is retried RETRY_MS = 283 ms of the channel's own ring
later: 283 * 1e-3 * f_sf is no whole number in double for either rate.

HAND -- the hand-over of every channel type: 13-tap channels, ring 1 real samples on a 4.092 MHz IF (L1 C/A, SBAS),
ring 2 int8 IQ (G1 with positive and negative frequency number, an RTL-SDR replay channel with ppmerr 30)."""
import numpy as np

import acq_cases as ac

CTYPE_L1CA, CTYPE_G1, CTYPE_SBAS = 1, 20, 27
FEND_FRTLSDR = 8
NOCODEDOPPLER = 1.602e15        # f_cf given to synth.make_if: the folded FDMA / clock offset is no code Doppler

RINGS = {1: dict(dtype=2, f_sf=16.368e6, f_if=0.0), 2: dict(dtype=1, f_sf=20e6, f_if=4e6)}
N1, N2 = 16368, 20000
GRID_DEFAULT, GRID_COARSE, GRID_R2 = (7000, 200, 10), (3000, 500, 3), ac.B_GRID

# (name, ctype, prn / frequency number, ring, grid, Doppler Hz, code phase chips, t_on s; Doppler None: absent)
MIX = [
    ("l1_present", CTYPE_L1CA, 5, 1, GRID_DEFAULT, 1517.0, 311.3, None),
    ("l1_absent", CTYPE_L1CA, 9, 1, GRID_DEFAULT, None, None, None),
    ("sbas", CTYPE_SBAS, 120, 1, GRID_DEFAULT, -830.0, 100.2, None),
    ("l1_late", CTYPE_L1CA, 30, 1, GRID_DEFAULT, -120.0, 555.5, 0.24),
    ("l1_intg3", CTYPE_L1CA, 12, 1, GRID_COARSE, 1040.0, 12.8, None),
    ("r2_l1_present", CTYPE_L1CA, 17, 2, GRID_R2, 2210.0, 640.7, None),
    ("r2_l1_absent", CTYPE_L1CA, 22, 2, GRID_R2, None, None, None),
    ("r2_g1_present", CTYPE_G1, 2, 2, GRID_R2, -1530.0, 77.4, None),
    ("r2_g1_late", CTYPE_G1, -3, 2, GRID_R2, 905.0, 402.9, 0.12),
]
MIX_CN0 = 47.0
MIX_SEED = {1: 431, 2: 422}     # (chosen so that every search keeps acq_cases.MARGIN on the oracle)
NSTEP = 12
C1, C2 = int(0.1 * 16.368e6), int(0.08 * 20e6)
FIRST_PUSH1 = 6 * N1
R2_STEPS = [3, 4, 5, 7, 8, 10, 11]              # the steps that push ring 2
RETRY_MS = 283
MAX_PERIODS = 130
# attempt (1-based) at which the oracle must acquire the channel; None: never
MIX_ACQUIRED_AT = dict(l1_present=1, l1_absent=None, sbas=1, l1_late=2, l1_intg3=1, r2_l1_present=1, r2_l1_absent=None,
                       r2_g1_present=1, r2_g1_late=2)
# the steps in which each channel is searched, as the schedule of DESIGN.md section 3.2a gives them
MIX_DUE = dict(l1_present=[1], l1_absent=[1, 4, 7, 10], sbas=[1], l1_late=[1, 4], l1_intg3=[0], r2_l1_present=[3],
               r2_l1_absent=[3, 8], r2_g1_present=[3], r2_g1_late=[3, 8])


def mix_wrpos():
    """[(write position of ring 1, of ring 2)] at each step."""
    out, w2 = [], 0
    for k in range(NSTEP):
        if k in R2_STEPS:
            w2 += C2
        out.append((FIRST_PUSH1 + k * C1, w2))
    return out


def first_try(spec):
    """(intg + 1) * nsamp (ref src/sdracq.c:24-26)."""
    return (spec[4][2] + 1) * (N1 if spec[3] == 1 else N2)


def retry_samples(ring):
    """The pause after a failed search, in samples of the channel's ring: the documented formula, in double."""
    return int(RETRY_MS * 1e-3 * RINGS[ring]["f_sf"])


def due_steps(spec, acquired_at):
    """The steps at which gnsscorr_rx_step must search the channel."""
    out, next_try = [], first_try(spec)
    for k, wps in enumerate(mix_wrpos()):
        wp = wps[spec[3] - 1]
        if wp >= next_try and wp >= first_try(spec):
            out.append(k)
            if acquired_at is not None and len(out) == acquired_at:
                break
            next_try = wp + retry_samples(spec[3])
    return out


def _foffset(ctype, prn):
    return 0.5625e6 * prn if ctype == CTYPE_G1 else 0.0


def _sats(gc, specs, ring, seed, cn0, extra_offset=None):
    rng = np.random.default_rng(seed)
    codes, sats = {}, []
    for i, s in enumerate(specs):
        name, ctype, prn, r, _, dop, cph, t_on = s[:8]
        if r != ring or dop is None:
            continue
        codes[name] = gc.gencode(prn, ctype)
        off = _foffset(ctype, prn) + (extra_offset or {}).get(name, 0.0)
        d = dict(prn=name, doppler=off + dop, codephase=cph, cn0=cn0, phase=0.4 * i,
                 bits=rng.choice([-1.0, 1.0], size=64))
        if t_on is not None:
            d["t_on"] = t_on
        sats.append(d)
    return codes, sats


def mix_signal(gc, synth, ring):
    """The whole recording of one ring."""
    fe = RINGS[ring]
    n = FIRST_PUSH1 + (NSTEP - 1) * C1 if ring == 1 else len(R2_STEPS) * C2
    codes, sats = _sats(gc, MIX, ring, MIX_SEED[ring], MIX_CN0)
    return synth.make_if(codes, n, f_sf=fe["f_sf"], f_if=fe["f_if"], dtype=fe["dtype"], sats=sats, seed=MIX_SEED[ring],
                         f_cf=NOCODEDOPPLER)


def mix_channel(gc, spec, **kw):
    name, ctype, prn, ring, (hband, step, intg) = spec[:5]
    return gc.Channel(prn, ctype=ctype, ftype=ring, hband=hband, step=step, intg=intg, **RINGS[ring], **kw)


def mix_oracle_channel(orc, spec, **kw):
    name, ctype, prn, ring, (hband, step, intg) = spec[:5]
    fe = RINGS[ring]
    return ac.grid(orc.make_chan(prn, ctype=ctype, dtype=fe["dtype"], f_sf=fe["f_sf"], f_if=fe["f_if"], **kw), hband, step, intg)


# ---- HAND ------------------------------------------------------------------------------------------------------------
HAND_RINGS = {1: dict(dtype=1, f_sf=16.368e6, f_if=4.092e6), 2: dict(dtype=2, f_sf=16.368e6, f_if=0.0)}
HAND_TAPS = dict(corrn=6, corrd=3, corrp=6)
RTL_PPMERR = 30
HAND = [
    ("l1_13tap", CTYPE_L1CA, 5, 1, GRID_DEFAULT, 1517.0, 311.3, None),
    ("sbas", CTYPE_SBAS, 120, 1, GRID_DEFAULT, -830.0, 100.2, None),
    ("l1_unlisted", CTYPE_L1CA, 12, 1, GRID_DEFAULT, -3222.0, 12.8, None),
    ("l1_absent", CTYPE_L1CA, 9, 1, GRID_DEFAULT, None, None, None),
    ("g1_plus", CTYPE_G1, 2, 2, GRID_DEFAULT, 1210.0, 77.4, None),
    ("g1_minus", CTYPE_G1, -3, 2, GRID_DEFAULT, -2330.0, 402.9, None),
    ("rtlsdr", CTYPE_L1CA, 25, 2, GRID_DEFAULT, 640.0, 870.1, None),
    ("g1_absent", CTYPE_G1, 5, 2, GRID_DEFAULT, None, None, None),
]
HAND_LISTED = [0, 1, 3, 4, 5, 6, 7]
HAND_ACQUIRED = [0, 1, 4, 5, 6]
HAND_SEED = {1: 511, 2: 512}
HAND_NPER = {1: 2130, 2: 230}       # ring 1 runs past period 2000, where the SBAS channel finds its symbol edge
HAND_WRPOS = 14 * N1
HAND_RUNS = (200, 1900)
RTL_OFFSET = 1575.42e6 * RTL_PPMERR * 1e-6


def hand_kw(spec):
    return dict(HAND_TAPS, fend=FEND_FRTLSDR, ppmerr=RTL_PPMERR) if spec[0] == "rtlsdr" else dict(HAND_TAPS)


def hand_signal(gc, synth, ring):
    fe = HAND_RINGS[ring]
    codes, sats = _sats(gc, HAND, ring, HAND_SEED[ring], 47.0, extra_offset={"rtlsdr": RTL_OFFSET})
    return synth.make_if(codes, HAND_NPER[ring] * N1, f_sf=fe["f_sf"], f_if=fe["f_if"], dtype=fe["dtype"], sats=sats,
                         seed=HAND_SEED[ring], f_cf=NOCODEDOPPLER)


def hand_channel(gc, spec):
    name, ctype, prn, ring = spec[:4]
    return gc.Channel(prn, ctype=ctype, ftype=ring, **HAND_RINGS[ring], **hand_kw(spec))


def hand_oracle_channel(orc, spec):
    name, ctype, prn, ring = spec[:4]
    fe = HAND_RINGS[ring]
    return orc.make_chan(prn, ctype=ctype, dtype=fe["dtype"], f_sf=fe["f_sf"], f_if=fe["f_if"], **hand_kw(spec))
