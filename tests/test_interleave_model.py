"""The interleaver / scrambler model of tests/interleave_model.py against the
802.11a facts it is pinned to, and the reason the interleaver exists: a notch
over adjacent carriers on the coded link of tests/fec_model.py (no GPU)."""

import numpy as np
import pytest

import fec_model as F
import interleave_model as IM
import oracle as O
from common import ALL_CONFIGS, D, EXTRA


def test_fixed_points_of_the_80211a_interleaver():
    p = IM.perm(48, 16, 1)
    assert list(p[:16]) == list(range(0, 48, 3))
    assert list(p[16:18]) == [1, 4]
    p = IM.perm(192, 16, 2)
    assert list(p[:6]) == [0, 13, 24, 37, 48, 61]
    assert p[15] == 181
    assert list(p[16:20]) == [1, 12, 25, 36]


def sweep():
    for n in list(range(8, 200, 8)) + [256, 600 - 600 % 8, 1024, 1536, 8192, 32768]:
        for c in range(1, n + 1):
            if n % c or (n > 600 and c not in (1, 12, 16, n)):
                continue
            for s in (1, 2, 3, 4):
                if IM.valid(n, c, s):
                    yield n, c, s


def test_bijection_and_closed_form_inverse():
    count = 0
    for n, c, s in sweep():
        p, inv = IM.perm(n, c, s), IM.inverse_perm(n, c, s)
        assert np.array_equal(np.sort(p), np.arange(n)), (n, c, s)
        assert np.array_equal(inv[p], np.arange(n)), (n, c, s)
        assert np.array_equal(p[inv], np.arange(n)), (n, c, s)
        count += 1
    assert count > 300


def test_interleave_and_deinterleave_are_inverse_and_blockwise():
    rng = np.random.default_rng(2)
    for n, c, s in ((8, 1, 1), (48, 16, 1), (96, 16, 3), (192, 12, 4), (1024, 16, 2)):
        x = rng.integers(-128, 128, (3, 5 * n)).astype(np.int8)
        y = IM.interleave(x, n, c, s)
        assert np.array_equal(IM.deinterleave(y, n, c, s), x)
        assert np.array_equal(y[1, 2 * n:3 * n][IM.perm(n, c, s)], x[1, 2 * n:3 * n])  # out[j(q)] = in[q]
        assert np.array_equal(IM.interleave(IM.deinterleave(x, n, c, s), n, c, s), x)


def test_invalid_parameters():
    for n, c, s in ((0, 1, 1), (4, 1, 1), (12, 1, 1), (32776, 1, 1), (48, 5, 1), (48, 0, 1), (48, 16, 2),
                    (48, 16, 0), (64, 128, 1)):
        assert not IM.valid(n, c, s), (n, c, s)
    assert IM.valid(8, 8, 1) and IM.valid(32768, 16, 4)


def test_every_test_config_has_a_valid_default_block():
    assert len(ALL_CONFIGS) == 16
    for name, p in ALL_CONFIGS.items():
        k = p["mod_type"]
        assert IM.valid(p["num_data_subc"] * k, 16, max(k // 2, 1)), name


def test_scrambler_sequence():
    s = IM.scramble_sequence(127, 3 * 127)
    assert "".join(map(str, s[:32])) == "00001110" "11110010" "11001001" "00000010"
    assert np.array_equal(s[:127], s[127:254]) and np.array_equal(s[:127], s[254:])
    assert int(s[:127].sum()) == 64
    for shift in range(1, 127):  # the period is 127, no shorter
        assert not np.array_equal(s[:127], s[shift:shift + 127])
    seen = set()
    for seed in range(1, 128):  # every seed: a different phase of the same sequence
        q = IM.scramble_sequence(seed, 127)
        assert int(q.sum()) == 64
        seen.add(q.tobytes())
    assert len(seen) == 127


def test_scramble_is_self_inverse_and_reduces_seeds():
    bits = np.random.default_rng(3).integers(0, 2, (5, 300), dtype=np.uint8)
    seeds = np.array([1, 127, 0, 128, 255], np.uint8)
    y = IM.scramble(bits, seeds)
    assert np.array_equal(IM.scramble(y, seeds), bits)
    assert not np.array_equal(y, bits)
    assert [IM.reduce_seed(v) for v in (0, 1, 127, 128, 254, 255)] == [127, 1, 127, 1, 127, 1]
    assert np.array_equal(y[2], bits[2] ^ IM.scramble_sequence(127, 300))
    assert np.array_equal(IM.scramble(bits, 5)[4], bits[4] ^ IM.scramble_sequence(5, 300))


# ------------------------------------------------------------------ the notch
def notch_case(p, rate, first, count, ncw=16, amp=8):
    """One codeword per frame, exact +-amp LLRs, the LLRs of `count` adjacent
    carriers from `first` zeroed in every symbol. Returns the number of
    codewords decoded wrongly (without, with) the per-symbol interleaver."""
    g = O.geometry(p)
    k = p["mod_type"]
    n, c, s = p["num_data_subc"] * k, 16, max(k // 2, 1)
    cap = g["bytes_per_frame"] * 8
    nb = F.max_info_bits(cap, rate)
    info = np.random.default_rng(1).integers(0, 2, (ncw, nb), dtype=np.uint8)
    frame = np.zeros((ncw, cap), np.uint8)
    coded = F.encode(info, rate)
    frame[:, :coded.shape[1]] = coded
    wrong = []
    for interleaved in (False, True):
        tx = IM.interleave(frame, n, c, s) if interleaved else frame
        llr = (amp * (1 - 2 * tx.astype(np.int64))).reshape(ncw, -1, n)
        llr[:, :, first * k:(first + count) * k] = 0
        llr = llr.reshape(ncw, cap)
        if interleaved:
            llr = IM.deinterleave(llr, n, c, s)
        bits, _ = F.viterbi(llr, nb, rate)
        wrong.append(int(np.any(bits != info, axis=1).sum()))
    return tuple(wrong)


@pytest.mark.parametrize("rate", [F.R12, F.R23])
def test_notch_of_five_carriers_on_N128_k4_s3(rate):
    """D = 64, 16-QAM, 3 symbols: 20 worthless LLRs in a row per symbol break
    every codeword; spread by the interleaver they break none."""
    assert notch_case(EXTRA["N128_k4_s3"], rate, 21, 5) == (16, 0)


def test_notch_of_six_carriers_on_config_D():
    assert notch_case(D, F.R12, 21, 6, ncw=4) == (4, 0)
