"""The correlation monitor (include/gnsscorr.h), restated rule by rule in numpy float64: the only
expected-value source of the monitor's tests.  Every arithmetic statement below is one IEEE double operation per
element (numpy adds, multiplies and divides float64 element by element, correctly rounded, and fuses nothing), so the
device has to agree bit for bit.  Not a conftest."""
import numpy as np

NTAP, NPAIR = 33, 16
TAPS = ("sI", "sQ", "aI", "aQ", "aP", "cfI", "cfQ", "cfP")
PAIRS = ("delta", "ratio")
SCALARS = ("win_cnt", "open", "n", "k", "bits", "nbad", "alarm", "alarms", "windows", "worst_pair")
FIELDS = TAPS + PAIRS + SCALARS


def zero_state():
    st = {f: np.zeros(NTAP) for f in TAPS}
    st.update({f: np.zeros(NPAIR) for f in PAIRS})
    st.update({f: 0 for f in SCALARS})
    return st


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def prm(kbits=0, skip_bits=0, nbad=1, npair=1, dtol=0.0, rtol=0.0, dref=(), rref=()):
    """The parameters as a dict, dref / rref filled up to 16 values with 0."""
    d, r = np.zeros(NPAIR), np.zeros(NPAIR)
    d[:len(dref)] = dref
    r[:len(rref)] = rref
    return dict(kbits=kbits, skip_bits=skip_bits, nbad=nbad, npair=npair, dtol=float(dtol), rtol=float(rtol), dref=d, rref=r)


def run(st, p, rate, corrn, II, QQ, flagsync, navbit, ndone, cnt0, events=None):
    """One channel, rows e < ndone of one run whose row 0 is the period with cnt == cnt0.  st: a dict with FIELDS,
    updated in place and returned.  p: prm(...); kbits 0: off, nothing is touched.  II / QQ: [nper][1 + 2 corrn].
    events (a list): gets ("window", cnt, delta[:corrn], ratio[:corrn], P, bad, worst, alarm) for every closed window."""
    if p["kbits"] == 0:
        return st
    R, T = int(rate), 1 + 2 * int(corrn)
    II, QQ = np.asarray(II, np.float64), np.asarray(QQ, np.float64)
    with np.errstate(all="ignore"):
        for e in range(int(ndone)):
            c = int(cnt0) + e
            if c == 0:
                st.update(zero_state())
            if flagsync[e] == 0:
                continue
            if st["open"]:
                st["sI"][:T] = st["sI"][:T] + II[e, :T]
                st["sQ"][:T] = st["sQ"][:T] + QQ[e, :T]
                st["n"] += 1
            if navbit[e] != 0:
                if st["open"] and st["n"] == R:
                    st["bits"] += 1
                    if st["bits"] > p["skip_bits"]:
                        d = np.float64(1.0 if navbit[e] > 0 else -1.0)
                        wi = d * st["sI"][:T]
                        wq = d * st["sQ"][:T]
                        ii = st["sI"][:T] * st["sI"][:T]
                        qq = st["sQ"][:T] * st["sQ"][:T]
                        pw = ii + qq
                        st["aI"][:T] = st["aI"][:T] + wi
                        st["aQ"][:T] = st["aQ"][:T] + wq
                        st["aP"][:T] = st["aP"][:T] + pw
                        st["k"] += 1
                        if st["k"] == p["kbits"]:
                            _close(st, p, corrn, c, events)
                st["open"], st["n"] = 1, 0
                st["sI"][:] = 0.0
                st["sQ"][:] = 0.0
    return st


def _close(st, p, corrn, c, events):
    for a, f in (("aI", "cfI"), ("aQ", "cfQ"), ("aP", "cfP")):
        st[f][:] = st[a]
    st["win_cnt"] = c
    st["windows"] += 1
    cf = st["cfI"]
    P = cf[0]
    for j in range(1, NPAIR + 1):
        if j <= corrn and P > 0:
            dm = cf[2 * j - 1] - cf[2 * j]
            sm = cf[2 * j - 1] + cf[2 * j]
            st["delta"][j - 1] = dm / P
            st["ratio"][j - 1] = sm / P
        else:
            st["delta"][j - 1] = st["ratio"][j - 1] = 0.0
    bad = not (P > 0)
    worst = 0
    for j in range(1, p["npair"] + 1):
        dd = st["delta"][j - 1] - p["dref"][j - 1]
        dr = st["ratio"][j - 1] - p["rref"][j - 1]
        if abs(dd) > p["dtol"] or abs(dr) > p["rtol"]:
            bad = True
            if worst == 0:
                worst = j
    st["worst_pair"] = worst
    st["nbad"] = st["nbad"] + 1 if bad else 0
    st["alarm"] = 1 if st["nbad"] >= p["nbad"] else 0
    st["alarms"] += st["alarm"]
    if events is not None:
        events.append(("window", c, st["delta"][:corrn].copy(), st["ratio"][:corrn].copy(), float(P), bool(bad), worst, st["alarm"]))
    for a in ("aI", "aQ", "aP"):
        st[a][:] = 0.0
    st["k"] = 0


def to_struct(st, rec):
    """Writes the dict st into one element (numpy void) of an array of CfmState."""
    for f in TAPS + PAIRS:
        rec[f][:] = st[f]
    for f in SCALARS:
        rec[f] = st[f]


def to_prm_struct(p, rec):
    """Writes the dict p into one element of an array of CfmPrm."""
    for f in ("kbits", "skip_bits", "nbad", "npair", "dtol", "rtol"):
        rec[f] = p[f]
    rec["dref"][:] = p["dref"]
    rec["rref"][:] = p["rref"]


def from_struct(rec):
    out = {f: np.array(rec[f], np.float64) for f in TAPS + PAIRS}
    out.update({f: int(rec[f]) for f in SCALARS})
    return out


def same(st, rec):
    """Every field of the dict st equal to the CfmState element rec, doubles as bytes; returns what differs."""
    bad = []
    for f in TAPS + PAIRS:
        a, b = np.asarray(st[f], np.float64), np.asarray(rec[f], np.float64)
        if a.tobytes() != b.tobytes():
            for t in range(len(a)):
                if a[t].tobytes() != b[t].tobytes():
                    bad.append((f, t, float(a[t]), float(b[t])))
    for f in SCALARS:
        if int(st[f]) != int(rec[f]):
            bad.append((f, int(st[f]), int(rec[f])))
    if "pad" in (rec.dtype.names or ()) and int(rec["pad"]) != 0:
        bad.append(("pad", 0, int(rec["pad"])))
    return bad
