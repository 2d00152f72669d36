"""The numpy model of the frequency-selective channel path (csi_model.py)
against the physics it models, on the CPU: noiseless, the least-squares
estimate is the channel itself and equalising with it restores the sent
points; with noise at a spectral notch, the channel-state weight is what lets
the decoder through, and the unit-phasor estimate does not equalise at all."""
import numpy as np
import pytest

import csi_model as CM
import fec_model as F
import oracle as O
import soft_model as SM
from common import D, EXTRA, TAPS_ECHO, TAPS_NOTCH, _apply_taps, cfg, payload

CONFIGS = {"N64_k1": EXTRA["N64_k1"], "N128_k4_s3": EXTRA["N128_k4_s3"], "D": D,
           "D384": cfg(D, num_data_subc=384), "D_pr2": cfg(D, num_pr_symb=2)}
TAPS = {"echo": TAPS_ECHO, "notch": TAPS_NOTCH}


def noiseless_region(p, taps, seed=3):
    g = O.geometry(p)
    data = payload(g["bytes_per_frame"], seed)
    fr = _apply_taps(O.frame_write(p, data), taps)
    t2 = p["t2sin_size"]
    return fr[t2:t2 + g["preamble_len"] + g["message_len"]], data


@pytest.mark.parametrize("taps", list(TAPS))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_noiseless_estimate_is_the_channel_and_equalises(name, taps):
    p = CONFIGS[name]
    g = O.geometry(p)
    k, S = p["mod_type"], p["num_symb"]
    region, data = noiseless_region(p, TAPS[taps])
    H, csi = CM.ls_estimate(p, region[:g["preamble_len"]])
    ratio = H / CM.tap_response(p, TAPS[taps])
    mean = ratio.mean()
    spread = float(np.abs(ratio - mean).max() / abs(mean))
    print(f"{name} {taps}: H / DFT(taps) = {mean:.6f}, spread {spread:.2e}")
    assert spread <= 1e-12
    assert abs(mean.imag) <= 1e-12 * abs(mean) and mean.real > 0, "the constant is not real"
    assert np.array_equal(csi, H.real ** 2 + H.imag ** 2)
    E = O.ofdm_fft(p, region[g["preamble_len"]:], S=S) / np.tile(H, S)
    sent = O.mod(k, data)[:len(E)]
    err = float(np.abs(E - sent).max())
    print(f"{name} {taps}: max |pts/H - sent| = {err:.2e}")
    assert err <= 1e-12
    assert np.array_equal(O.demod(k, E)[0], data)


def test_smoothing_windows():
    rng = np.random.default_rng(5)
    n, half = 32, 16
    raw = rng.normal(size=n) + 1j * rng.normal(size=n)
    assert np.array_equal(CM.smooth_halves(raw, 0), raw)
    H = CM.smooth_halves(raw, 3)
    # inside a half the full window; clipped at both ends of both halves
    windows = {8: (5, 12), 0: (0, 4), 2: (0, 6), 15: (12, 16), 13: (10, 16), 16: (16, 20), 17: (16, 21),
               31: (28, 32), 29: (26, 32), 24: (21, 28)}
    for c, (a, b) in windows.items():
        assert abs(H[c] - raw[a:b].mean()) <= 1e-15, c
    for w in (half, half + 1, 64):  # w >= D/2: each half its mean
        H = CM.smooth_halves(raw, w)
        assert np.allclose(H[:half], raw[:half].mean(), rtol=0, atol=1e-15)
        assert np.allclose(H[half:], raw[half:].mean(), rtol=0, atol=1e-15)


def test_ls_estimate_smooth_is_the_smoothed_raw_estimate():
    p = EXTRA["N128_k4_s3"]
    region, _ = noiseless_region(p, TAPS_ECHO)
    raw, _ = CM.ls_estimate(p, region)
    for w in (1, 3, 64):
        H, csi = CM.ls_estimate(p, region, w)
        assert np.array_equal(H, CM.smooth_halves(raw, w))
        assert np.array_equal(csi, H.real ** 2 + H.imag ** 2)


@pytest.mark.parametrize("k", SM.KS)
def test_csi_llr_weights_and_erasures(k):
    rng = np.random.default_rng(k)
    Dn, S = 8, 3
    pts = (rng.uniform(-3, 3, (2, Dn * S)) + 1j * rng.uniform(-3, 3, (2, Dn * S)))
    assert np.array_equal(CM.csi_llr(k, pts, np.ones(Dn), 2.0), SM.ref_llr(k, pts, 2.0))
    w = rng.uniform(0.01, 4, (2, Dn))
    L = CM.csi_llr(k, pts, w, 2.0)
    assert np.array_equal(L, SM.ref_llr(k, pts, 2.0 * np.tile(w, S)))
    assert np.array_equal(CM.csi_llr(k, pts, w[0], 1.0)[1], SM.ref_llr(k, pts[1], np.tile(w[0], S)))
    bad_pts = pts.copy()
    bad_pts[0, 1] = complex(np.nan, 0.5)
    bad_pts[0, 2] = complex(0.5, np.inf)
    bad_pts[1, 3] = complex(-np.inf, np.nan)
    bad_w = w.copy()
    bad_w[0, 4], bad_w[0, 5], bad_w[1, 6], bad_w[1, 7] = 0.0, -1.0, np.inf, np.nan
    Lb = CM.csi_llr(k, bad_pts, bad_w, 2.0)
    erased = np.zeros(pts.shape, bool)
    erased[0, 1] = erased[0, 2] = erased[1, 3] = True
    erased[0, 4::Dn] = erased[0, 5::Dn] = erased[1, 6::Dn] = erased[1, 7::Dn] = True
    assert np.all(Lb[erased] == 0.0) and not np.signbit(Lb[erased]).any(), "an erasure is not +0.0"
    assert np.array_equal(Lb[~erased], L[~erased])
    assert np.isfinite(Lb).all()


# ------------------------------------------------------------------ why the feature exists
def test_csi_weight_carries_the_code_through_a_notch():
    """N128_k4_s3, notch, rate 1/2, 32 frames, 18 dB: the zero-forced points
    of the weak carriers are as much noise as signal. Unweighted the decoder
    believes them (21 of 32 codewords lost with this generator, 15 with
    another realisation of the same set-up); weighted by |H|^2 it loses none. The
    control must lose at least 8, and at least 4 times the CSI leg's + 4."""
    case = CM.link_case(EXTRA["N128_k4_s3"], TAPS_NOTCH, F.R12, 32, 18.0)
    lost_ls, hard_ls, _ = CM.link_decode(case, "ls")
    lost_csi, hard_csi, _ = CM.link_decode(case, "csi")
    print(f"codewords lost of 32: LS unweighted {lost_ls}, LS + CSI {lost_csi}; hard errors {hard_ls}")
    assert hard_ls == hard_csi  # the same equalised points
    assert lost_csi == 0
    assert lost_ls >= 8
    assert lost_ls >= 4 * lost_csi + 4


def test_unit_phasor_estimate_loses_every_codeword_noiseless():
    case = CM.link_case(EXTRA["N128_k4_s3"], TAPS_NOTCH, F.R12, 8, None)
    lost_unit, hard_unit, _ = CM.link_decode(case, "unit")
    lost_ls, hard_ls, _ = CM.link_decode(case, "ls")
    print(f"noiseless: unit phasors lose {lost_unit} of 8 ({hard_unit} hard errors), LS {lost_ls} ({hard_ls})")
    assert lost_unit == 8 and hard_unit > 1000
    assert (lost_ls, hard_ls) == (0, 0)
