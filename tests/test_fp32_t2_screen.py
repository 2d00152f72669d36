"""The walker's FP32 T2 screen (ofdm_sync.hip stream_walk_kernel, ofdm_fft32.hpp)
decides a block from FP32 only when its detector ratio clears the level by
t2_margin = 4e-5. The margin rests on an error model, not a proof (DESIGN.md
4.1): a transform error ||X^ - X||_2 <= e ||X||_2 with e = 9 log2(N) u = 81 u
at N = 512, u = 2^-24, moves either energy sum by at most (2 e + e^2 + 15 u)
relative (the squares of the perturbed bins, and 15 u for the sums' own
roundings), and the ratio of two such sums by twice that: 2.1e-5. The model's inequality is checked on the device's own arithmetic in
tests/test_gpu_fft_accuracy.py (the transform, <= 5.1 u measured) and
tests/test_gpu_walk_bounds.py (the ratio, <= 3.0e-7 measured), and on the
real walker in tests/test_gpu_t2_near_level.py. Here, on the CPU: the figure
is recomputed from its formula and held against the product's default margin
and the margin below which ofdm_set_walk_tuning refuses; and the size of an
FP32 transform's ratio error is observed with numpy's FP32 FFT against FP64
on noise, on the T2 symbol's tones and on partial overlaps of the two (the
decision-relevant case), at the stream's amplitude scales. No GPU code runs."""
import os
import sys

import ctypes as C

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle as O  # noqa: E402

MARGIN = 4e-5


def ratio(x, mask, dtype):
    X = np.fft.fft(x.astype(dtype))
    e = (X.real.astype(X.real.dtype) ** 2 + X.imag ** 2)
    return float(np.sum(e * mask, dtype=e.dtype) / np.sum(e, dtype=e.dtype))


def test_fp32_ratio_error_is_far_below_the_margin():
    p = dict(O.DEFAULT)
    n, f1, f2, sm = p["t2sin_size"], p["t2_sin_f1"], p["t2_sin_f2"], p["smooth"]
    k = np.arange(n)
    mask = (((k >= f1 - sm) & (k <= f1 + sm)) | ((k >= f2 - sm) & (k <= f2 + sm))).astype(np.float64)
    t2 = O.t2_symbol(p)
    rng = np.random.default_rng(7)
    worst = 0.0
    for trial in range(400):
        scale = 10.0 ** rng.uniform(-2, 4)
        noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale * rng.uniform(0.01, 1.0)
        shift = int(rng.integers(0, n))
        block = noise.copy()
        block[shift:] += np.asarray(t2)[: n - shift] * scale  # a block that overlaps the T2 symbol partly
        r64 = ratio(block, mask, np.complex128)
        r32 = ratio(block, mask.astype(np.float32), np.complex64)
        worst = max(worst, abs(r32 - r64))
    assert worst < MARGIN / 20, worst


def model_ratio_bound(n=512, u=2.0 ** -24):
    """The error model's bound on the FP32 detector ratio (module docstring)."""
    e = 9 * np.log2(n) * u
    return 2 * (2 * e + e * e + 15 * u)


def test_margin_covers_the_error_model():
    import ofdm_mi355x as M
    bound = model_ratio_bound()
    assert 2.10e-5 < bound < 2.12e-5  # the documented 2.1e-5
    t = M.WalkTuning()
    M.check(M.lib().ofdm_walk_tuning_default(C.byref(t)))
    assert t.t2_f32 == 1 and t.allow_uncertified == 0
    assert t.t2_margin >= bound
    # the refusal threshold: a margin just below the model's bound, and one just below the default, are refused
    # without allow_uncertified. The range checks run before the context is touched and nothing is stored on a
    # refusal; the context here is scratch memory (no GPU, no real context), large enough for a store all the same.
    scratch = C.create_string_buffer(1 << 20)
    for margin in (np.nextafter(bound, 0.0), np.nextafter(t.t2_margin, 0.0)):
        bad = M.WalkTuning()
        M.check(M.lib().ofdm_walk_tuning_default(C.byref(bad)))
        bad.t2_margin = float(margin)
        assert M.lib().ofdm_set_walk_tuning(C.cast(scratch, C.c_void_p), C.byref(bad)) != 0
    assert bytes(scratch) == bytes(1 << 20)  # refused: nothing written
