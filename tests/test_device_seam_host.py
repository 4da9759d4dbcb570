"""The device-seam cases on the oracle alone (no GPU): tests/device_seam_cases.py can tell a reader that is ordered behind
the ring's writer from one that is not.

In-ring condition: every period of every batch lies inside what the ring holds when the batch is issued -- not ahead of
the write position, not more than a ring behind it -- so the engine's ring check stays silent and nothing reads a slot
that is being rewritten.

Sensitivity condition: for every batch and every chunk the batch reads, the oracle run again with that chunk replaced by
what its slot held before (zeros on the first lap, the chunk four earlier afterwards) differs from the true sums in at
least one period of every channel.  Each of those chunks was written by the caller on its stream (the two resident ones
too, in tests/test_gpu_device_seam.py), so a correlator that is not ordered behind the caller's writes cannot pass.
The chunk batch k's caller writes just before it, k + 2, is by construction never read by batch k (asserted below: the
reader trails the writer by a chunk, as in multigpu.py's ring schedule), so replacing it changes nothing; the condition
is therefore stated over the chunks a batch does read, the newest of which is k + 1, written one batch earlier with no
host synchronisation in between."""
import numpy as np
import pytest

import device_seam_cases as dc


@pytest.mark.parametrize("inst", sorted(dc.INSTANCES))
def test_every_period_lies_inside_what_the_ring_holds(gc, orc, synth, inst):
    exp = dc.expected(gc, orc, synth, inst)
    assert [b["II"].shape for b in exp["batches"]] == [(4, n, dc.NTAP) for n in dc.BATCHES]
    for k, b in enumerate(exp["batches"]):
        wp = dc.wrpos_at(k)
        first, last = b["loc"].astype(np.int64), b["loc"].astype(np.int64) + b["ns"]
        assert (last <= wp).all(), (k, int(last.max()), wp)                     # written already
        assert (first >= wp - dc.RINGLEN).all(), (k, int(first.min()), wp)      # not overwritten yet
        # the slot being written while batch k + 1 is issued -- chunk k + 3 over chunk k - 1 -- is not read by batch k,
        # which may still be running then
        assert (first >= k * dc.CHUNK).all(), (k, int(first.min()))
        # and the chunk written in front of batch k is ahead of everything it reads
        assert dc.chunks_read(exp, k)[-1] < dc.RESIDENT + k, (k, dc.chunks_read(exp, k))
    # start states below one period; the chain is continuous from batch to batch
    assert all(0 < st["buffloc"] < dc.NSAMP for st in dc.start_states(gc, inst))
    for a, b in zip(exp["batches"][:-1], exp["batches"][1:]):
        assert np.array_equal(a["loc"][:, -1].astype(np.int64) + a["ns"][:, -1], b["loc"][:, 0].astype(np.int64))
    assert [st["buffloc"] for st in exp["state"]] == \
        [int(l) + int(n) for l, n in zip(exp["batches"][-1]["loc"][:, -1], exp["batches"][-1]["ns"][:, -1])]
    # eight chunks through four slots: every slot is overwritten once, and the batches read both laps
    assert sorted({c for k in range(len(dc.BATCHES)) for c in dc.chunks_read(exp, k)}) == list(range(7))


@pytest.mark.parametrize("inst", sorted(dc.INSTANCES))
def test_a_stale_slot_changes_every_channel_of_every_batch(gc, orc, synth, inst):
    exp = dc.expected(gc, orc, synth, inst)
    for k, b in enumerate(exp["batches"]):
        read = dc.chunks_read(exp, k)
        assert k in read and k + 1 in read, (k, read)
        for c in read:
            II, QQ = dc.stale_batch(gc, orc, synth, inst, k, c)
            for ch in range(II.shape[0]):
                bad = [e for e in range(II.shape[1])
                       if not (np.array_equal(II[ch, e], b["II"][ch, e]) and np.array_equal(QQ[ch, e], b["QQ"][ch, e]))]
                assert bad, (inst, "batch", k, "chunk", c, "channel", ch, "a stale slot gives the true sums")
        # a chunk the batch does not read leaves it alone (the comparison above is not vacuous the other way round)
        II, QQ = dc.stale_batch(gc, orc, synth, inst, k, dc.RESIDENT + k)
        assert np.array_equal(II, b["II"]) and np.array_equal(QQ, b["QQ"]), k


def test_the_two_instances_differ(gc, orc, synth):
    a, b = (dc.expected(gc, orc, synth, i) for i in ("A", "B"))
    assert not np.array_equal(dc.stream(gc, synth, "A"), dc.stream(gc, synth, "B"))
    assert all(not np.array_equal(x["II"], y["II"]) for x, y in zip(a["batches"], b["batches"]))
