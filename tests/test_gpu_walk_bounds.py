"""The stream walker's two certified error bounds, checked on the device's own
arithmetic through the test-only library (c-ofdm_amd/devtest, tests/devtest.py).

T2 ratio. The FP32 screen (ofdm_sync.hip stream_walk_kernel, the t2_f32
branch) decides a block from sa/ta alone when it clears the level by t2_margin
= 4e-5; the model behind the margin bounds the ratio's error
by 2.1e-5. Here sa/ta and sb/tb of the launcher's replica of that branch
(fft_regs_wave32p, the 2-bit mask weights, the packed energies, group_sum) are
compared with the longdouble ratio of the same f64 block, for N = 64..512,
three masks (the default config's; two overlapping ranges, weight 2; ranges
clipped at bin 0 and bin N-1) and the blocks on which a ratio can go wrong:
partial overlaps of the T2 symbol, a mask tone beside a tone at the bin next
to the mask edge, mask energy 1e-6 of the total, ratios within +-1e-4 of the
level, int16-valued blocks up to full scale, scales 1e-3 .. 3e4. The screen's
verdict is "uncertain" for a total of 0, below 1e-20, above 1e30, inf and NaN,
and never a certain PASS or FAIL that the longdouble ratio contradicts.

Correlation. walk_preamble_fft certifies each lag with |e^ - e| <= 1024 u
||x||_2 max|tspec|, u = 2^-24 for its FP32 tier (fft_regs_wave32c, c_mulw) and
2^-53 for the FP64 pass (fft_regs_wave, cmul). The window pass of both is
compared with the longdouble circular correlation on windows of a real frame
at its preamble, the template itself, one 3e4 sample among 1e-3 noise,
full-scale int16 values and short windows, for the default config's template
spectrum and a random spectrum with one dominant bin."""
import numpy as np
import pytest

import devtest as dt
import oracle as O
from common import D, payload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LEVEL = D["t2_sin_level"] / 1000
MARGIN = 4e-5          # ofdm_walk_tuning_default().t2_margin
RATIO_BOUND = 2.1e-5   # the model's figure (tests/test_fp32_t2_screen.py recomputes it)
LD = dt.LD


def masks(n):
    sm, f1, f2 = D["smooth"], D["t2_sin_f1"], D["t2_sin_f2"]
    clip = lambda f: (max(0, f - sm), min(n - 1, f + sm))  # noqa: E731  (as ofdm_tables.hpp builds the ranges)
    return {"default": clip(f1) + clip(f2), "overlap": clip(f1) + clip(f1 + sm + 1), "clipped": clip(2) + clip(n - 3)}


def tone(n, b, ampl=1.0):
    j = np.arange(n)
    return ampl * np.exp(2j * np.pi * ((b * j) % n) / n)


def cnoise(rng, n, scale):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale


def blocks(n, mask, rng):
    """The block families of the module docstring for one size and mask:
    (rows, family names)."""
    a1, b1, a2, b2 = mask
    c1, c2 = (a1 + b1) // 2, (a2 + b2) // 2
    weights = dt.t2_mask(n, mask)
    edge = next(k for k in range(b1 + 1, n) if not weights[k])  # the bin next to the mask edge (f1 + smooth + 1)
    t2 = tone(n, c1) + tone(n, c2)
    rows, fam = [], []

    def add(name, x):
        rows.append(np.asarray(x, np.complex128))
        fam.append(name)

    for scale in (1e-3, 1.0, 200.0, 3e4):
        for trial in range(12):  # the family of tests/test_fp32_t2_screen.py
            x = cnoise(rng, n, scale * rng.uniform(0.01, 1.0))
            shift = int(rng.integers(0, n))
            x[shift:] += t2[: n - shift] * scale
            add("overlap", x)
        for a in (0.5, 1.0, 1.9, 2.0, 2.1, 4.0):  # a^2 / (a^2 + 1): 0.2 .. 0.94, around the level at a = 2
            add("edge", scale * (a * tone(n, c1) + tone(n, edge)))
        add("mask1e-6", scale * (1e-3 * tone(n, c1) + tone(n, edge)))
        add("mask1e-6", scale * 1e-3 * tone(n, c2) + cnoise(rng, n, scale / np.sqrt(2 * n)))
        for delta in np.linspace(-1e-4, 1e-4, 9):  # ratio = a^2 / (a^2 + 1) = level + delta
            r = LEVEL + delta
            add("near", scale * (np.sqrt(r / (1 - r)) * tone(n, c1) + tone(n, edge)))
            w = cnoise(rng, n, 1.0)  # white: n sum|w|^2 off-mask-ish energy, the ratio lands near the level
            W = np.fft.fft(w)
            m = dt.t2_mask(n, mask)
            em, et = float(np.sum(m * np.abs(W) ** 2)), float(np.sum(np.abs(W) ** 2))
            # (a^2 n^2 + em) / (a^2 n^2 + et) = r, the cross term of the tone with w's bin c1 left to chance
            a = np.sqrt(max((r * et - em) / (1 - r), 0.0)) / n
            add("near-noise", scale * (a * tone(n, c1) + w))
    for amp in (100.0, 3000.0, 32767.0 / 3.3):  # int16-valued, up to full scale
        x = amp * (2.0 * tone(n, c1) + tone(n, edge)) + cnoise(rng, n, amp * 0.05)
        add("int16", np.clip(np.round(x.real), -32767, 32767) + 1j * np.clip(np.round(x.imag), -32767, 32767))
        add("int16", rng.integers(-32767, 32768, n) + 1j * rng.integers(-32767, 32768, n))
        full = 32767.0 * np.exp(2j * np.pi * ((c1 * np.arange(n)) % n) / n)
        add("int16", np.round(full.real) + 1j * np.round(full.imag))
    return np.stack(rows), np.array(fam)


@pytest.mark.parametrize("logt", [6, 7, 8, 9])
def test_fp32_t2_ratio_within_the_model_bound(logt):
    n = 1 << logt
    rng = np.random.default_rng(40 + logt)
    worst = {}
    for name, mask in masks(n).items():
        x, fam = blocks(n, mask, rng)
        if len(x) % 2:
            x, fam = x[:-1], fam[:-1]
        ref = dt.t2_ratio_ref(x, mask)
        h = len(x) // 2
        # first half in lane A beside the second half in lane B, then swapped: every block in both lanes
        for swap in (False, True):
            xa, xb = (x[h:], x[:h]) if swap else (x[:h], x[h:])
            _, _, sums, verdict = dt.fft32p(logt, xa, xb, mask, LEVEL, MARGIN)
            ra = sums[:, 1] / sums[:, 0]  # float32 division, as the screen's
            rb = sums[:, 3] / sums[:, 2]
            got = np.concatenate([rb, ra] if swap else [ra, rb])
            ver = np.concatenate([verdict[:, 1], verdict[:, 0]] if swap else [verdict[:, 0], verdict[:, 1]])
            err = np.abs(got.astype(LD) - ref).astype(np.float64)
            for f in np.unique(fam):
                worst[(name, f)] = max(worst.get((name, f), 0.0), float(err[fam == f].max()))
            w = int(err.argmax())
            assert err.max() <= RATIO_BOUND, (name, fam[w], w, float(got[w]), float(ref[w]))
            # a certain verdict agrees with the reference's decision (ratio > level)
            passes = (ref > LD(LEVEL))
            assert not np.any((ver == 1) & ~passes), (name, np.nonzero((ver == 1) & ~passes)[0])
            assert not np.any((ver == 0) & passes), (name, np.nonzero((ver == 0) & passes)[0])
            # and the verdict is the rule applied to the returned sums
            lev, marg = np.float32(LEVEL), np.float32(MARGIN)
            want = np.where(got > lev + marg, 1, np.where(got <= lev - marg, 0, 2))
            assert np.array_equal(ver, want)
    print(f"\nT2 ratio N={n}: worst |r32 - r| {max(worst.values()):.3e} (bound {RATIO_BOUND:.1e}); by mask and family: "
          + ", ".join(f"{k[0]}/{k[1]} {v:.2e}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("logt", [6, 7, 8, 9])
def test_screen_is_uncertain_outside_the_normal_range(logt):
    n = 1 << logt
    mask = masks(n)["default"]
    c1 = (mask[0] + mask[1]) // 2
    base = tone(n, c1) + 0.1 * tone(n, (mask[1] + 2) % n)  # ratio 0.99: a certain PASS at a normal scale
    rows = {
        "zero": np.zeros(n, np.complex128),
        "tiny": base * 1e-18,     # total ~ n^2 1e-36 < 1e-20
        "below": base * (0.5e-10 / n),  # total ~ 2.5e-21
        "huge": base * 1e14,      # total ~ n^2 1e28 > 1e30
        "inf": base * 1e18,       # |X|^2 overflows FP32
        "nan": np.where(np.arange(n) == 3, np.nan, base),
        "normal": base,
    }
    x = np.stack(list(rows.values()))
    for xa, xb, col in ((x, x[::-1], 0), (x[::-1], x, 1)):
        _, _, sums, verdict = dt.fft32p(logt, xa, xb, mask, LEVEL, MARGIN)
        v = dict(zip(rows, verdict[:, col]))
        tot = dict(zip(rows, sums[:, 2 * col]))
        assert tot["zero"] == 0 and 0 < tot["tiny"] < 1e-20 and 0 < tot["below"] < 1e-20 and 1e30 < tot["huge"] < np.inf
        assert np.isinf(tot["inf"]) and np.isnan(tot["nan"])
        assert all(v[k] == 2 for k in ("zero", "tiny", "below", "huge", "inf", "nan")), v
        assert v["normal"] == 1


# ---------------------------------------------------------------- correlation
M = 512


def template_spectrum(templ):
    """tspec_k = sum_j c_j e^{+2 pi i k j / M} in longdouble (as ofdm_tables.hpp
    builds it), so that IDFT(DFT(x) . tspec)_i = sum_j x[i + j] c_j."""
    c = np.zeros(M, dt.CLD)
    c[: len(templ)] = templ
    return dt.dft_ref(c, +1)


def windows(rng):
    g = O.geometry(D)
    templ = O.preamble_setup(D)[2]
    L = len(templ)
    fr = O.frame_write(D, payload(g["bytes_per_frame"], 5))
    t2 = D["t2sin_size"]
    rows, fam = [], []

    def add(name, x, w=M):
        v = np.zeros(M, np.complex128)
        v[:w] = np.asarray(x)[:w]
        rows.append(v)
        fam.append(name)

    for off in (-64, -1, 0, 1, 97):  # the preamble at lag 64, 1, 0 / just missed
        add("frame", fr[t2 + off: t2 + off + M])
        add("frame-mult", fr[t2 + off: t2 + off + M] * D["mult"])
    add("template", np.conj(templ), L)
    add("template", templ, L)
    x = cnoise(rng, M, 1e-3)
    x[200] = 3e4
    add("spike", x)
    add("int16", rng.integers(-32767, 32768, M) + 1j * rng.integers(-32767, 32768, M))
    add("int16", np.full(M, 32767.0 - 32767.0j))
    for w in (L, L + 1, 300, M - 1):  # short windows: W < M, zero tail
        add("short", fr[t2: t2 + M] * D["mult"], w)
    return np.stack(rows), np.array(fam), templ


@pytest.mark.parametrize("f32", [True, False], ids=["fp32-tier", "fp64-pass"])
def test_fft_correlation_within_the_certified_bound(f32):
    rng = np.random.default_rng(77)
    x, fam, templ = windows(rng)
    u = 2.0 ** -24 if f32 else 2.0 ** -53
    Hr = cnoise(rng, M, 1.0)
    Hr[37] = 400.0 - 300.0j  # one dominant bin
    for name, H in (("template", template_spectrum(templ)), ("dominant-bin", Hr.astype(dt.CLD))):
        H64 = H.astype(np.complex128)  # what the context uploads (rounded once from longdouble)
        ref = dt.dft_ref(dt.dft_ref(x, -1) * H64.astype(dt.CLD), +1) / LD(M)
        if name == "template":  # the same by the definition: sum_j x[(i + j) mod M] c_j
            idx = (np.arange(M)[:, None] + np.arange(len(templ))[None, :]) % M
            direct = np.sum(x.astype(dt.CLD)[:, idx] * templ.astype(dt.CLD)[None, None, :], axis=-1)
            assert float(np.abs(direct - ref).max() / np.abs(ref).max()) < 1e-15
        got = dt.corr(f32, x, H64).astype(dt.CLD) / LD(M)
        err = np.abs(got - ref).max(axis=-1).astype(np.float64)
        bound = 1024.0 * u * np.sqrt(np.sum(np.abs(x) ** 2, axis=-1)) * float(np.abs(H64).max())
        use = err / bound
        w = int(use.argmax())
        print(f"\ncorrelation {'FP32' if f32 else 'FP64'} H={name}: worst error / bound {use[w]:.3e} "
              f"(headroom {1 / use[w]:.1f}x, {fam[w]} row {w})")
        assert np.all(np.isfinite(err))
        assert np.all(err <= bound), (name, fam[w], w, err[w], bound[w])
