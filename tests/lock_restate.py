"""The lock detector of the receiver schedule (include/gnsscorr.h), restated line by line in plain
Python: the only expected-value source of the lock monitor's tests.  Python floats are IEEE doubles and every statement
below is one operation, so the device has to agree bit for bit."""
import numpy as np

FIELDS = ("sI", "sQ", "w", "npsum", "mu_last", "lost_cnt", "open", "n", "k", "nbad", "lost", "reason", "windows", "pad")


def zero_state():
    return dict(sI=0.0, sQ=0.0, w=0.0, npsum=0.0, mu_last=0.0, lost_cnt=0, open=0, n=0, k=0, nbad=0, lost=0, reason=0,
                windows=0, pad=0)


def run(st, prm, rate, I, Q, flagsync, navbit, ndone, cnt0, events=None):
    """One channel, rows e < ndone of one run whose row 0 is the period with cnt == cnt0.  st: a dict with FIELDS,
    updated in place and returned.  prm: dict(sync_periods, kbits, nbad, mu_min).  events (a list): gets
    ("np", cnt, np) for every whole bit, ("mu", cnt, mu) for every window and ("lost", cnt, reason)."""
    sync_periods, kbits, nbad, mu_min = prm["sync_periods"], prm["kbits"], prm["nbad"], float(prm["mu_min"])
    for e in range(int(ndone)):
        cnt = int(cnt0) + e
        if cnt == 0:
            st.update(zero_state())
        if st["lost"]:
            continue
        if flagsync[e] == 0:
            if sync_periods > 0 and cnt + 1 >= sync_periods:
                st["lost"], st["reason"], st["lost_cnt"] = 1, 1, cnt
                if events is not None:
                    events.append(("lost", cnt, 1))
            continue
        i, q = float(I[e]), float(Q[e])
        if st["open"]:
            st["sI"] = st["sI"] + i
            st["sQ"] = st["sQ"] + q
            ii = i * i
            qq = q * q
            st["w"] = st["w"] + (ii + qq)
            st["n"] += 1
        if navbit[e] != 0:
            if st["open"] and st["n"] == rate:
                a = st["sI"] * st["sI"]
                b = st["sQ"] * st["sQ"]
                np_ = (a + b) / st["w"] if st["w"] > 0 else 0.0
                if events is not None:
                    events.append(("np", cnt, np_))
                st["npsum"] = st["npsum"] + np_
                st["k"] += 1
                if st["k"] == kbits:
                    mu = st["npsum"] / float(kbits)
                    st["mu_last"] = mu
                    st["windows"] += 1
                    st["nbad"] = st["nbad"] + 1 if mu < mu_min else 0
                    st["k"] = 0
                    st["npsum"] = 0.0
                    if events is not None:
                        events.append(("mu", cnt, mu))
                    if st["nbad"] >= nbad:
                        st["lost"], st["reason"], st["lost_cnt"] = 1, 2, cnt
                        if events is not None:
                            events.append(("lost", cnt, 2))
            st["open"], st["n"] = 1, 0
            st["sI"] = st["sQ"] = st["w"] = 0.0
    return st


def to_struct(st, rec):
    """Writes the dict st into one element (numpy void) of an array of LockState."""
    for f in FIELDS:
        rec[f] = st[f]


def from_struct(rec):
    out = {}
    for f in FIELDS:
        v = rec[f]
        out[f] = float(v) if isinstance(v, (float, np.floating)) else int(v)
    return out


def same(st, rec):
    """Every field of the dict st equal to the LockState element rec, doubles bit for bit; returns the names that differ."""
    bad = []
    for f in FIELDS:
        a, b = st[f], rec[f]
        if isinstance(a, float):
            if np.float64(a).tobytes() != np.float64(b).tobytes():
                bad.append((f, a, float(b)))
        elif int(a) != int(b):
            bad.append((f, a, int(b)))
    return bad
