"""bench.py --dump-outputs: what the last timed step computed, written as float64 .npy files (a stand-in engine: no
GPU involved)."""
import numpy as np

import bench


class _Engine:
    """trk_fetch() / trk_get_state() shaped as the package's Engine returns them."""

    def __init__(self, nch=4, ne=1000, nt=5, seed=3):
        rng = np.random.default_rng(seed)
        self.II = rng.integers(-2**20, 2**20, size=(nch, ne, nt)).astype(np.float64)
        self.QQ = rng.integers(-2**20, 2**20, size=(nch, ne, nt)).astype(np.float64)
        self.ns = rng.integers(16367, 16370, size=(nch, ne)).astype(np.int32)
        self.st = [dict(carrfreq=100.5 * i, codefreq=1.023e6 + i, remcode=0.25, remcarr=-0.5, buffloc=2**40 + i)
                   for i in range(nch)]

    def trk_fetch(self):
        return self.II.copy(), self.QQ.copy(), self.ns.copy()

    def trk_get_state(self):
        return [dict(s) for s in self.st]


def _load(d, name):
    a = np.load(d / (name + ".npy"))
    assert a.dtype == np.float64, name
    return a


def test_dump_outputs_whole(tmp_path):
    eng = _Engine()
    names = bench.dump_outputs(str(tmp_path), eng)
    assert sorted(p.stem for p in tmp_path.glob("*.npy")) == names
    assert np.array_equal(_load(tmp_path, "trk_II"), eng.II)
    assert np.array_equal(_load(tmp_path, "trk_QQ"), eng.QQ)
    assert np.array_equal(_load(tmp_path, "trk_nsamp"), eng.ns)
    assert np.array_equal(_load(tmp_path, "trk_periods"), np.arange(eng.II.shape[1]))
    for k in ("carrfreq", "codefreq", "remcode", "remcarr", "buffloc"):
        assert np.array_equal(_load(tmp_path, "state_" + k), [s[k] for s in eng.st]), k


def test_dump_outputs_sampled_under_the_cap(tmp_path):
    eng = _Engine()
    per_period = 4 * (2 * 5 + 1) * 8
    cap = (1 << 20) + 100 * per_period
    bench.dump_outputs(str(tmp_path / "a"), eng, cap_bytes=cap)
    bench.dump_outputs(str(tmp_path / "b"), eng, cap_bytes=cap)
    p = _load(tmp_path / "a", "trk_periods").astype(int)
    assert len(p) == 100 and np.all(np.diff(p) > 0)
    assert np.array_equal(_load(tmp_path / "a", "trk_II"), eng.II[:, p])
    assert np.array_equal(_load(tmp_path / "a", "trk_nsamp"), eng.ns[:, p])
    assert sum(f.stat().st_size for f in (tmp_path / "a").glob("*.npy")) <= cap
    for f in (tmp_path / "a").glob("*.npy"):            # the same sample every time
        assert np.array_equal(np.load(f), np.load(tmp_path / "b" / f.name)), f.name
