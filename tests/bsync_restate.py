"""Bit synchronisation by symbol energy (include/gnsscorr.h), restated rule by rule in plain Python: the
only expected-value source of the detector's tests.  Python floats are IEEE doubles and every statement below is one
operation, so the device has to agree bit for bit.  Not a conftest."""
import numpy as np

ARRAYS = ("E", "sI", "sQ", "fill")
SCALARS = ("ratio_last", "a0", "decided_cnt", "armed", "n", "tests", "done", "best", "synci")
FIELDS = ARRAYS + SCALARS
NOFF = 20


def zero_state():
    return dict(E=[0.0] * NOFF, sI=[0.0] * NOFF, sQ=[0.0] * NOFF, fill=[0] * NOFF, ratio_last=0.0, a0=0, decided_cnt=0,
                armed=0, n=0, tests=0, done=0, best=0, synci=0)


def copy_state(st):
    return {k: (list(v) if isinstance(v, list) else v) for k, v in st.items()}


def run(st, prm, rate, I, Q, flagsync, ndone, cnt0, events=None):
    """One channel, rows e < ndone of one run whose row 0 is the period with cnt == cnt0.  st: a dict with FIELDS,
    updated in place and returned.  prm: dict(start_cnt, nsym, nsym_max, gate); nsym 0: off, nothing is touched.
    events (a list): gets ("test", cnt, n, best offset, ratio, passed) for every test."""
    start_cnt, nsym, nsym_max, gate = prm["start_cnt"], prm["nsym"], prm["nsym_max"], float(prm["gate"])
    R = int(rate)
    if nsym == 0:
        return st
    for e in range(int(ndone)):
        c = int(cnt0) + e
        if c == 0:                                                  # 1
            st.update(zero_state())
        if st["done"]:                                              # 2
            break
        if flagsync[e] != 0:                                        # 3
            st["done"] = 3
            break
        if c < start_cnt:                                           # 4
            continue
        if not st["armed"]:                                         # 5
            st["armed"], st["a0"] = 1, c
        i, q = float(I[e]), float(Q[e])
        E, sI, sQ, fill = st["E"], st["sI"], st["sQ"], st["fill"]
        for o in range(R):                                          # 6
            if fill[o] > 0 or c % R == o:
                sI[o] = sI[o] + i
                sQ[o] = sQ[o] + q
                fill[o] += 1
                if fill[o] == R:
                    a = sI[o] * sI[o]
                    b = sQ[o] * sQ[o]
                    E[o] = E[o] + (a + b)
                    sI[o] = sQ[o] = 0.0
                    fill[o] = 0
        L = c - st["a0"] + 1                                        # 7
        if (L + 1) % R == 0:
            n = st["n"] = (L + 1) // R - 1
            if n >= 1 and n % nsym == 0:
                best = 0
                for o in range(1, R):
                    if E[o] > E[best]:
                        best = o
                h = (best + R // 2) % R
                st["tests"] += 1
                st["ratio_last"] = E[best] / E[h] if E[h] > 0 else 0.0
                passed = E[best] > 0 and E[best] >= gate * E[h]
                if events is not None:
                    events.append(("test", c, n, best, st["ratio_last"], bool(passed)))
                if passed:
                    st["done"], st["best"], st["synci"], st["decided_cnt"] = 1, best, (best + R - 1) % R, c
                elif n >= nsym_max:
                    st["done"] = 2
    return st


def layout_synci(first_period, cnt0, rate):
    """The true synci of a channel whose row 0 (sdrthread's cnt = cnt0) holds code period `first_period` of a
    synth.make_if layout with symbol_periods = rate (symbol s spans the code periods rate*s .. rate*s + rate - 1): the
    cnt mod rate of a symbol's last period, as tests/sync_if_cases.py::synci states it."""
    return (cnt0 + rate - 1 - first_period) % rate


def to_struct(st, rec):
    """Writes the dict st into one element (numpy void) of an array of BsyncState."""
    for f in ARRAYS:
        rec[f][:] = st[f]
    for f in SCALARS:
        rec[f] = st[f]


def from_struct(rec):
    out = {}
    for f in ARRAYS:
        out[f] = [float(v) if f != "fill" else int(v) for v in rec[f]]
    for f in SCALARS:
        v = rec[f]
        out[f] = float(v) if isinstance(v, (float, np.floating)) else int(v)
    return out


def _same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def same(st, rec):
    """Every field of the dict st equal to the BsyncState element rec, doubles bit for bit; returns what differs."""
    bad = []
    for f in ARRAYS:
        for o in range(NOFF):
            a, b = st[f][o], rec[f][o]
            if (not _same_bits(a, b)) if isinstance(a, float) else int(a) != int(b):
                bad.append((f, o, a, b.item()))
    for f in SCALARS:
        a, b = st[f], rec[f]
        if (not _same_bits(a, b)) if isinstance(a, float) else int(a) != int(b):
            bad.append((f, a, b.item()))
    return bad
