"""Brute-force numpy model of the soft demapper (include/ofdm_mi355x.h, "soft
decisions"): max-log LLRs of the reference's constellation by searching every
level, in FP64. The reference for the soft-decision tests; pinned to the
oracle's hard decisions in test_soft_model.py.

    L_b = s * ( min_{c: bit_b(c)=1} |z-c|^2 - min_{c: bit_b(c)=0} |z-c|^2 )

QAM is separable (symbol = col | row*m, natural binary per axis): bits
0..k/2-1 from the imaginary axis, k/2..k-1 from the real axis, MSB first.
Levels as the reference computes them (modulation.cpp:19): 2/(m-1)*j - 1."""
import numpy as np

KS = (1, 2, 4, 6, 8)


def levels(k):
    m = 1 << (k // 2)
    return 2.0 / (m - 1) * np.arange(m, dtype=np.float64) - 1.0


def _axis_minima(x, h):
    """(min over levels with bit b = 0, with bit b = 1), each (..., h), b MSB first."""
    m = 1 << h
    lv = 2.0 / (m - 1) * np.arange(m, dtype=np.float64) - 1.0
    d = (x[..., None] - lv) ** 2  # (..., m)
    j = np.arange(m)
    d0 = np.empty(x.shape + (h,))
    d1 = np.empty(x.shape + (h,))
    for b in range(h):
        one = ((j >> (h - 1 - b)) & 1) == 1
        d0[..., b] = d[..., ~one].min(axis=-1)
        d1[..., b] = d[..., one].min(axis=-1)
    return d0, d1


def minima(k, pts):
    """(d0, d1): per point and bit, the squared distance to the nearest
    constellation point whose bit b is 0 / 1. Shapes pts.shape + (k,)."""
    pts = np.asarray(pts, np.complex128)
    if k == 1:
        r = np.sqrt(0.5)
        c0, c1 = complex(-r, -r), complex(r, r)  # psk(i, 5*pi/4, 2), modulation.cpp:28-30
        d0 = (pts.real - c0.real) ** 2 + (pts.imag - c0.imag) ** 2
        d1 = (pts.real - c1.real) ** 2 + (pts.imag - c1.imag) ** 2
        return d0[..., None], d1[..., None]
    h = k // 2
    r0, r1 = _axis_minima(pts.imag, h)
    c0, c1 = _axis_minima(pts.real, h)
    return np.concatenate([r0, c0], axis=-1), np.concatenate([r1, c1], axis=-1)


def ref_llr(k, pts, scale=1.0):
    """LLRs, shape pts.shape + (k,). `scale` broadcasts against pts (a
    per-frame scale for pts of shape (nframes, npts): shape (nframes, 1))."""
    d0, d1 = minima(k, pts)
    s = np.asarray(scale, np.float64)
    return s[..., None] * (d1 - d0)


def quant_i8(L):
    """OFDM_LLR_I8: clamp(rint(L), -127, 127), rint half-to-even."""
    return np.clip(np.rint(L), -127, 127).astype(np.int8)


def f32_bar(L_ref, abs_bar):
    """|L_gpu - L_ref| allowed for OFDM_LLR_F32: the absolute bar of the FP64
    evaluation plus one f32 rounding."""
    return abs_bar + 2.0 ** -23 * np.abs(L_ref)


def check_f32(got, L_ref, abs_bar, what=""):
    err = np.abs(got.astype(np.float64) - L_ref)
    bar = f32_bar(L_ref, abs_bar)
    worst = float((err - bar).max())
    print(f"{what} f32: max |err| {err.max():.3e}, max err/bar {float((err / np.maximum(bar, 1e-300)).max()):.3f}")
    assert worst <= 0.0, f"{what}: f32 LLR off its bar by {worst:.3e}"


def check_i8(got, L_ref, abs_bar, max_excluded=1e-4, designed=None, what=""):
    """|q_gpu - q_ref| <= 1 everywhere; equal wherever L_ref is farther than
    abs_bar from a half-integer and from +-127.5. At most max_excluded of the
    values (not counting the `designed` ones: boolean mask of values built to
    sit on such a boundary) may lie in the excluded set."""
    q = quant_i8(L_ref).astype(np.int32)
    g = got.astype(np.int32)
    assert np.abs(g - q).max() <= 1, f"{what}: an int8 LLR differs by more than 1"
    frac = np.abs(L_ref - np.floor(L_ref) - 0.5)  # distance from the nearest half-integer
    near = frac <= abs_bar
    near |= np.abs(np.abs(L_ref) - 127.5) <= abs_bar
    count = near if designed is None else near & ~designed
    share = float(count.sum()) / max(count.size, 1)
    print(f"{what} i8: {int(near.sum())} of {near.size} values within {np.max(abs_bar):.1e} of a rounding boundary "
          f"({int(count.sum())} not designed), {int((g != q).sum())} differ by 1")
    assert share <= max_excluded, f"{what}: {share:.2e} of the values are excluded from the equality check"
    assert np.array_equal(g[~near], q[~near]), f"{what}: an int8 LLR differs away from a rounding boundary"
