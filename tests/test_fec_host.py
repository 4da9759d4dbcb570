"""The restatement the GPU decoder and frame replay are held to (fec_restate.py), held to known answers itself: no GPU,
no library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fec_restate as fr  # noqa: E402
import sbas_cases as sc  # noqa: E402


def _codeword(seed):
    bits = np.concatenate([np.random.default_rng(seed).integers(0, 2, size=750), np.zeros(6, np.int64)])
    return bits[:750], fr.encode(bits)


def spaced_errors(seed, n=1512):
    """Symbol indices at least 64 apart, none in the first or last 64 symbols."""
    rng = np.random.default_rng(1000 + seed)
    idx, i = [], 64 + int(rng.integers(0, 64))
    while i < n - 64:
        idx.append(i)
        i += 64 + int(rng.integers(0, 64))
    return np.array(idx)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_clean_decode_returns_the_bits(seed):
    bits, sym = _codeword(seed)
    assert sym.size == fr.WIN and set(np.unique(sym)) == {-1, 1}
    assert np.array_equal(fr.viterbi27(sym, 750), bits)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_spaced_single_errors_are_corrected(seed):
    bits, sym = _codeword(seed)
    idx = spaced_errors(seed)
    assert idx.size >= 10 and idx.min() >= 64 and idx.max() < 1512 - 64 and np.diff(idx).min() >= 64
    bad = sym.copy()
    bad[idx] = -bad[idx]
    assert np.array_equal(fr.viterbi27(bad, 750), bits)


def test_batch_axis_changes_nothing():
    rng = np.random.default_rng(4)
    w = (1 - 2 * rng.integers(0, 2, size=(5, 44))).astype(np.int8)
    w[2, :9] = 0
    both = fr.viterbi27(w, 16)
    for i in range(5):
        assert np.array_equal(both[i], fr.viterbi27(w[i], 16))
    # the polynomial pair is live: swapped, the same symbols decode differently
    assert not np.array_equal(fr.viterbi27(w, 16, fr.POLYB, fr.POLYA), both)


def test_encoder_inverts_with_its_input():
    """Both polynomials have odd weight, so a complemented bit stream encodes to the complemented symbols once the
    register is full: what lets a stream of polarity -1 decode to complemented bits."""
    bits = np.random.default_rng(5).integers(0, 2, size=100)
    a, b = fr.encode(bits, state=0), fr.encode(1 - bits, state=63)
    assert np.array_equal(a, -b)


def _crc24q_bytes(data):
    """The same CRC in the layout the reference checks: bytewise over the right-aligned 29 bytes."""
    crc = 0
    for byte in data:
        crc ^= byte << 16
        for _ in range(8):
            crc <<= 1
            if crc & 0x1000000:
                crc ^= 0x1864CFB
    return crc & 0xFFFFFF


def test_crc24q_known_answers():
    assert _crc24q_bytes(b"123456789") == 0xCDE703            # the published check value (CRC-24/LTE-A = CRC-24Q)
    assert fr.crc24q([int(c) for byte in b"123456789" for c in format(byte, "08b")]) == 0xCDE703
    assert fr.crc24q([0] * 226) == 0


def test_message_builder_crc():
    rng = np.random.default_rng(6)
    bodies = [np.zeros(212, np.int64), np.ones(212, np.int64)] + [rng.integers(0, 2, size=212) for _ in range(20)]
    for i, body in enumerate(bodies):
        m = fr.sbas_message(i, i % 64, body)
        assert len(m) == 250 and m[:8] == fr._bits(fr.PREAMBLES[i % 3], 8) and m[8:14] == fr._bits(i % 64, 6)
        right_aligned = np.packbits(np.array([0] * 6 + m[:226], np.uint8)).tobytes()
        assert len(right_aligned) == 29
        assert _crc24q_bytes(right_aligned) == int("".join(map(str, m[226:])), 2)
    m = fr.sbas_message(0, 12, bodies[2], tow=sc.TOW, week=sc.WEEK)
    assert int("".join(map(str, m[107:127])), 2) + 1 == sc.TOW and int("".join(map(str, m[127:137])), 2) + 1024 == sc.WEEK


@pytest.mark.parametrize("name", ["pol+1_lead0", "pol+1_lead7", "pol-1_lead0", "pol-1_lead7"])
def test_replay_finds_the_frame(name):
    case, rep, (navbit, buffloc, cnts, locs, _) = sc.replayed(name)
    k = case["found"]
    assert rep.flagsyncf == 1 and rep.flagtow == 1 and rep.flagdec == 1 and rep.flagpol == 0
    assert rep.polarity == case["polarity"]
    assert rep.firstsfcnt == cnts[k] and rep.firstsf == locs[k]
    assert rep.firstsftow == sc.TOW and rep.week == sc.WEEK
    # one update behind the frame: message 1 (type 2), a second later
    assert rep.id == 2 and rep.tow_gpst == sc.TOW + 1.0
    assert rep.msg[0] == 0x9A


def test_replay_takes_the_flagpol_branch():
    case, rep, (navbit, buffloc, cnts, locs, _) = sc.replayed("flagpol")
    assert rep.flagpol == 1 and rep.polarity == -1 and rep.flagdec == 1
    assert rep.firstsfcnt == cnts[case["found"]]
    assert rep.firstsftow == sc.TOW and rep.id == 12
    # the branch, step by step: the stream up to the false pair raises the flag and leaves no frame
    cut = 3 + 1511 + 2 * 20 + 1
    part = fr.SbasReplay()
    part.run(case["symbols"][:cut - 1], cnts[:cut - 1], locs[:cut - 1])
    assert part.flagpol == 0
    part.run(case["symbols"][cut - 1:cut], cnts[cut - 1:cut], locs[cut - 1:cut])
    assert part.flagpol == 1 and part.polarity == 1 and part.flagsyncf == 0 and part.flagtow == 0


def test_replay_without_time_and_with_aid():
    case, rep, _ = sc.replayed("noaid")
    assert rep.flagtow == 0 and rep.flagsyncf == 0 and rep.flagdec == 0 and rep.tow_gpst == 0 and rep.week == 0
    assert rep.id != 0                                      # it did decode messages
    case, rep, (navbit, buffloc, cnts, locs, aid) = sc.replayed("aid")
    k = case["found"]
    assert rep.flagdec == 1 and rep.firstsfcnt == cnts[k] and rep.week == sc.AID_WEEK
    assert rep.firstsftow == aid[cnts[k]]
    case, rep, _ = sc.replayed("noframe")
    assert rep.flagtow == 0 and rep.flagsyncf == 0 and rep.firstsfcnt == 0


def test_replay_in_pieces_is_the_same():
    case, whole, (navbit, buffloc, cnts, locs, _) = sc.replayed("pol+1_lead7")
    rep = fr.SbasReplay()
    for i in range(0, len(cnts), 333):
        rep.run(case["symbols"][i:i + 333], cnts[i:i + 333], locs[i:i + 333])
    assert rep.fields() == whole.fields() and np.array_equal(rep.fbits, whole.fbits)
