"""Pins tests/fec_model.py (the channel code's definition) to textbook facts:
the 133/171 impulse response, the puncture patterns, noiseless and
single-error decoding, and the tie rule."""
import numpy as np
import pytest

import fec_model as F

INFO_BITS = (1, 7, 8, 58, 59, 250)


def test_impulse_response():
    m = F.encode_mother(np.array([[1, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.uint8))[0]
    a, b = m[0::2], m[1::2]
    assert "".join(map(str, a[:7])) == "1011011"
    assert "".join(map(str, b[:7])) == "1111001"
    inter = np.array([int(c) for pair in zip("1011011", "1111001") for c in pair], np.uint8)
    assert np.array_equal(m[:14], inter)
    assert int(m.sum()) == 10 and not m[14:].any()


@pytest.mark.parametrize("rate", F.RATES)
def test_coded_bits_against_brute_force(rate):
    keep = F.KEEP[rate]
    for nb in list(range(1, 40)) + [58, 59, 250, 8186]:
        brute = sum(1 for i in range(2 * (nb + 6)) if keep[i % len(keep)])
        assert F.coded_bits(nb, rate) == brute
    assert F.coded_bits(8186, F.R12) == 16384


def test_puncture_positions():
    # rate 3/4 keeps A0 B0 A1 B2 of every three steps, 2/3 keeps A0 B0 A1
    assert list(F.kept_positions(6, F.R34)[:8]) == [0, 1, 2, 5, 6, 7, 8, 11]
    assert list(F.kept_positions(6, F.R23)[:6]) == [0, 1, 2, 4, 5, 6]
    assert list(F.kept_positions(1, F.R12)) == list(range(14))
    info = np.random.default_rng(0).integers(0, 2, (3, 30), dtype=np.uint8)
    m = F.encode_mother(info)
    assert np.array_equal(F.encode(info, F.R34)[:, :4], m[:, [0, 1, 2, 5]])


@pytest.mark.parametrize("rate", F.RATES)
@pytest.mark.parametrize("nb", INFO_BITS)
def test_noiseless_roundtrip(nb, rate):
    info = np.random.default_rng(nb * 10 + rate).integers(0, 2, (5, nb), dtype=np.uint8)
    c = F.encode(info, rate)
    for amp, dt in ((9, np.int64), (0.75, np.float64)):
        llr = ((1 - 2 * c.astype(np.int64)) * amp).astype(dt)
        got, best = F.viterbi(llr, nb, rate)
        assert np.array_equal(got, info)
        assert np.allclose(best, amp * c.shape[1])
        assert np.allclose(F.path_metric(got, llr, rate), best)


def test_every_single_flip_decodes():
    nb = 58
    info = np.random.default_rng(58).integers(0, 2, (1, nb), dtype=np.uint8)
    c = F.encode(info, F.R12)[0].astype(np.int64)
    n = len(c)
    llr = np.tile((1 - 2 * c) * 5, (n, 1))
    llr[np.arange(n), np.arange(n)] *= -1
    got, _ = F.viterbi(llr, nb, F.R12)
    assert np.array_equal(got, np.tile(info, (n, 1)))


def test_all_zero_llrs_follow_the_tie_rule():
    """info_bits = 1, T = 7, every LLR 0: every ACS between two reachable (or
    two unreachable) candidates is a tie and keeps j = 0; where only one is
    reachable, it wins. The traceback starts in state 0 at step 6, whose
    candidates p_0 = 0 and p_1 = 1 are both reachable after six steps (all 64
    states are) with metric 0: the tie keeps p_0 = 0. The same holds at steps
    5 .. 1 for state 0 (metrics 0 against 0, or 0 against unreachable), and at
    step 0 state 0's p_0 = 0 is the start itself. The path is 0 -> 0 -> ... ->
    0, whose info bit is 0."""
    for rate in F.RATES:
        got, best = F.viterbi(np.zeros((1, F.coded_bits(1, rate)), np.int64), 1, rate)
        assert got.tolist() == [[0]] and best[0] == 0
    got, _ = F.viterbi(np.zeros((2, F.coded_bits(59, F.R12))), 59, F.R12)
    assert not got.any()


def test_tie_rule_prefers_j0_between_equal_paths():
    """One non-zero LLR at mother bit A_0 against bit 0 (L = -4): the paths
    u_0 = 1 (A_0 = 1, gains 4, loses nothing elsewhere as all other LLRs are 0)
    win over u_0 = 0, so the output is not the all-zero word; the model then
    has to end in state 0 through ties alone."""
    nb = 8
    llr = np.zeros((1, F.coded_bits(nb, F.R12)), np.int64)
    llr[0, 0] = -4
    got, best = F.viterbi(llr, nb, F.R12)
    assert best[0] == 4 and got[0, 0] == 1
    assert F.path_metric(got, llr, F.R12)[0] == 4


def test_pack_unpack():
    bits = np.array([[1, 0, 0, 0, 0, 0, 0, 1, 1, 1]], np.uint8)
    assert F.pack(bits).tolist() == [[0x81, 0xC0]]
    assert np.array_equal(F.unpack(F.pack(bits), 10), bits)
