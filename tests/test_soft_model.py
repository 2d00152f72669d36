"""The brute-force LLR model (tests/soft_model.py) pinned to the oracle: its
signs are Modulation::demod's hard decisions, its same-bit minimum vanishes on
the constellation itself, and it is 4-Lipschitz in the point (the bound the
fused-path bars in test_gpu_soft.py rest on). CPU only."""
import numpy as np
import pytest

import oracle as O
import soft_model as SM


def point_bits(k, pts):
    """Modulation::demod's decisions, one row of k bits (MSB first) per point."""
    by, _ = O.demod(k, pts)
    return np.unpackbits(by)[:len(pts) * k].reshape(len(pts), k)


@pytest.mark.parametrize("k", SM.KS)
def test_sign_is_the_oracles_hard_decision(k):
    rng = np.random.default_rng(10 + k)
    n = 200_000
    pts = rng.uniform(-3, 3, n) + 1j * rng.uniform(-3, 3, n)
    L = SM.ref_llr(k, pts)
    bits = point_bits(k, pts)
    sure = np.abs(L) > 1e-12
    assert sure.mean() > 0.999
    assert np.array_equal((L < 0)[sure], bits[sure] == 1)


@pytest.mark.parametrize("k", SM.KS)
def test_same_bit_minimum_is_zero_on_the_constellation(k):
    con = O.constellation(k)
    d0, d1 = SM.minima(k, con)
    idx = np.arange(1 << k)
    bits = (idx[:, None] >> (k - 1 - np.arange(k))[None, :]) & 1
    assert np.array_equal(point_bits(k, con), bits)  # point i demodulates to i
    same = np.where(bits == 1, d1, d0)
    other = np.where(bits == 1, d0, d1)
    if k == 1:  # cos/sin(5*pi/4): the model's 1/sqrt(2) within an ulp
        assert same.max() < 1e-30
    else:
        assert np.all(same == 0.0)
    # the nearest point with the other bit is one level step away (BPSK: the other point)
    step2 = 4.0 if k == 1 else (2.0 / ((1 << (k // 2)) - 1)) ** 2
    assert abs(other.min() - step2) < 1e-12


@pytest.mark.parametrize("k", SM.KS)
def test_model_is_4_lipschitz(k):
    rng = np.random.default_rng(20 + k)
    n = 100_000
    z = rng.uniform(-3, 3, n) + 1j * rng.uniform(-3, 3, n)
    dz = (rng.normal(size=n) + 1j * rng.normal(size=n)) * 1e-3
    slope = np.abs(SM.ref_llr(k, z + dz) - SM.ref_llr(k, z)).max(axis=1) / np.abs(dz)
    assert slope.max() <= 4.0 * (1 + 1e-9)


def test_quantiser_rounds_half_to_even_and_saturates():
    L = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.5, 300.0, -127.49, -127.5, -1e9, 0.49999])
    assert SM.quant_i8(L).tolist() == [0, 2, 2, 0, -2, 126, 127, 127, -127, -127, -127, 0]
