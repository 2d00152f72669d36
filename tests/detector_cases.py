"""Fixtures of the stand-alone sync detectors' GPU tests
(tests/test_gpu_detectors.py: ofdm_t2_scan, ofdm_find_preamble,
ofdm_preamble_corr, ofdm_cfo_estimate on every kernel instance and edge; the
fixtures themselves are checked on the CPU in tests/test_detector_cases.py).
No torch, no GPU: numpy and the oracle.

- T2 cases: one config per t2_scan_kernel instance (T2sin_size 64 .. 4096,
  tones and smooth scaled from 17 / 51 / 5) and three mask-edge configs at 256
  (a band clipped at 0, one clipped at size - 1, overlapping bands); per config
  a 3-frame impaired stream, the same stream behind a block of exact zeros, one
  with a NaN sample and one with an Inf sample, and a list of (stream, n,
  start) scans.
- Preamble cases: (pr_sin_len, T2sin_size) pairs from one slice to nineteen,
  three stream textures each, a list of starts (negative, past n, n cut below
  the buffer, nothing in reach), and streams whose first passing lag has a
  ratio of level (1 +- d), d down to 1e-13.
- CFO cases: one form per cfo_kernel instance and five multi-symbol forms,
  4 impaired frames and 2 exact-tie frames each.
"""
import functools

import numpy as np

import oracle as O
from common import D, capture_stream, cfg as mkcfg, payload


# ------------------------------------------------------------------ references
def find_corr_ref(x, n, start, tpl, cycles):
    """PREAMBLE_FORM::find_corr in FP64: the running norm recurrence (the sum
    of the first L energies, then +|x[i+L]|^2 -|x[i]|^2 after each lag, in
    that order), the norm > 1 gate and |sum x[start+i+j] c_j| / sqrt(norm).
    Samples outside [0, n) read as zero. Returns (cor, norms)."""
    L = len(tpl)
    idx = start + np.arange(cycles + L)
    ok = (idx >= 0) & (idx < n)
    seg = np.zeros(cycles + L, np.complex128)
    seg[ok] = x[idx[ok]]
    en = seg.real * seg.real + seg.imag * seg.imag
    norm = 0.0
    for i in range(L):
        norm += float(en[i])
    norms = np.empty(cycles)
    for i in range(cycles):
        norms[i] = norm
        norm += float(en[i + L])
        norm -= float(en[i])
    corr = np.lib.stride_tricks.sliding_window_view(seg, L)[:cycles] @ tpl
    gate = norms > 1.0
    cor = np.zeros(cycles)
    cor[gate] = np.abs(corr[gate]) / np.sqrt(norms[gate])
    return cor, norms


def corr_profile(x, n, start, tpl, cycles):
    """find_corr_ref's (ratio, norms) by an FFT correlation and a cumulative
    sum, the ratio at every lag whatever its gate: within 1e-12 or so of the
    serial form, for the conditioning checks of many starts."""
    L = len(tpl)
    idx = start + np.arange(cycles + L)
    ok = (idx >= 0) & (idx < n)
    seg = np.zeros(cycles + L, np.complex128)
    seg[ok] = x[idx[ok]]
    m = 1 << int(cycles + 2 * L).bit_length()
    corr = np.fft.ifft(np.fft.fft(seg, m) * np.fft.fft(tpl[::-1], m))[L - 1: L - 1 + cycles]
    ps = np.concatenate([[0.0], np.cumsum(np.abs(seg) ** 2)])
    norms = ps[L: L + cycles] - ps[:cycles]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(norms > 0, np.abs(corr) / np.sqrt(np.abs(norms)), 0.0)
    return ratio, norms


def stream_with_marks(cfg, nf, seed, gap_max, tail=0, snr_db=20.0, cfo_max=0.004):
    """common.impaired_stream's recipe (full frames, random 0..gap_max zero
    gaps, per-frame CFO and phase, AWGN snr_db down over all) with `tail`
    more samples of noise alone at the end. Returns (samples, the T2 markers'
    first samples)."""
    g = O.geometry(cfg)
    rng = np.random.default_rng(seed)
    data = payload(nf * g["bytes_per_frame"], seed)
    parts = [np.zeros(int(rng.integers(0, gap_max + 1)), np.complex128)]
    marks, pos = [], len(parts[0])
    for f in range(nf):
        fr = O.frame_write(cfg, data[f * g["bytes_per_frame"]:(f + 1) * g["bytes_per_frame"]])
        i = np.arange(len(fr))
        fr = fr * np.exp(2j * np.pi * rng.uniform(-cfo_max, cfo_max) * i + 1j * rng.uniform(-np.pi, np.pi))
        gap = np.zeros(int(rng.integers(0, gap_max + 1)), np.complex128)
        marks.append(pos)
        pos += len(fr) + len(gap)
        parts += [fr, gap]
    parts.append(np.zeros(tail, np.complex128))
    return O.awgn(np.concatenate(parts), 10 ** (-snr_db / 20), seed=seed), marks


def capture_marks(cfg, x):
    """The markers' first samples in a common.capture_stream stream: its
    silences are exact zeros, and a T2 symbol's first sample is not."""
    g = O.geometry(cfg)
    marks, pos = [], 0
    while pos < len(x) and np.any(x[pos:] != 0):
        pos += int(np.argmax(x[pos:] != 0))
        marks.append(pos)
        pos += g["frame_len"]
    return marks


def t2_hits(cfg, x, marks):
    """The T2 hit of every frame: find_t2sin scanning from an eighth of a
    block before the marker (a scan whose grid splits a marker evenly between
    two blocks finds neither)."""
    hits = [O.find_t2sin(cfg, x, max(0, m - cfg["t2sin_size"] // 8)) for m in marks]
    assert all(m - cfg["t2sin_size"] <= h <= m + cfg["t2sin_size"] for h, m in zip(hits, marks)), (hits, marks)
    return hits


# ------------------------------------------------------------------ T2 cases
T2_SIZES = (64, 128, 256, 512, 1024, 2048, 4096)
T2_TONES = {64: (4, 13, 1), 128: (8, 25, 2), 256: (17, 51, 5), 512: (34, 102, 10), 1024: (68, 204, 20),
            2048: (136, 408, 40), 4096: (272, 816, 80)}  # (f1, f2, smooth): 17 / 51 / 5 scaled
T2_G = {64: 32, 128: 16, 256: 8, 512: 4, 1024: 2, 2048: 1, 4096: 1}  # t2_scan_kernel's blocks per workgroup


def t2_config(size, **kw):
    f1, f2, sm = T2_TONES[size]
    return mkcfg(D, num_symb=2, t2sin_size=size, t2_sin_f1=f1, t2_sin_f2=f2, smooth=sm, **kw)


T2_CONFIGS = {f"t2sin{s}": t2_config(s) for s in T2_SIZES}
T2_CONFIGS["low-edge"] = mkcfg(t2_config(256), t2_sin_f1=3)     # f1 - smooth < 0
T2_CONFIGS["high-edge"] = mkcfg(t2_config(256), t2_sin_f2=252)  # f2 + smooth > 255
T2_CONFIGS["overlap"] = mkcfg(t2_config(256), t2_sin_f2=24)     # |f1 - f2| <= 2 smooth: bins 19..22 count twice
T2_SEEDS = {k: 700 + i for i, k in enumerate(T2_CONFIGS)}
T2_HEAD = 5  # blocks before the stream in the "special" stream: noise, zeros, NaN, Inf, noise


@functools.lru_cache(maxsize=None)
def t2_case(key):
    """One config's streams and scans: dict(cfg, G, streams {name: samples},
    marks, scans [(tag, stream name, n, start)]). "plain" is the impaired
    stream, "special" the same behind T2_HEAD blocks: noise, exact zeros, noise
    with a NaN sample, noise with an Inf sample, noise."""
    cfg = T2_CONFIGS[key]
    T, G = cfg["t2sin_size"], T2_G[cfg["t2sin_size"]]
    x, marks = stream_with_marks(cfg, 3, T2_SEEDS[key], 2 * T)
    head = O.awgn(np.zeros(T2_HEAD * T, np.complex128), 0.1, seed=T2_SEEDS[key] + 50)
    head[T:2 * T] = 0.0
    head[2 * T + T // 3] = complex(np.nan, 0.3)
    head[3 * T + T // 5] = complex(0.2, -np.inf)
    xs = np.concatenate([head, x])
    n, ns = len(x), len(xs)
    late = marks[-1] + T  # the first sample after the last marker
    scans = [("plain-0", "plain", n, 0), ("plain-1", "plain", n, 1), ("plain-mid", "plain", n, T // 2 + 3),
             ("plain-late", "plain", n, late),
             ("no-block-0", "plain", T - 1, 0), ("no-block-mid", "plain", T // 2 + 3 + T - 1, T // 2 + 3),
             ("no-block-at-n", "plain", n, n), ("special-0", "special", ns, 0), ("special-1", "special", ns, 1),
             ("special-mid", "special", ns, T // 2 + 3),
             ("special-late", "special", ns, T2_HEAD * T + late),
             ("special-cut", "special", T2_HEAD * T - T // 4, 0)]  # the head alone, its last block cut: no hit
    # n cut so that the block count leaves a tail of dead groups in the last workgroup
    for tag, start in (("cut-0", 0), ("cut-1", 1)):
        nb = (n - start) // T
        k = (nb - 1) // G * G + 1 if G > 1 else nb - 1
        assert 0 < k <= nb
        scans.append((tag, "plain", start + k * T + T // 3, start))
    scans.append(("cut-one-block", "plain", 2 * T - 1, 0))
    for s in (x, xs):
        s.setflags(write=False)
    return dict(cfg=cfg, G=G, streams={"plain": x, "special": xs}, marks=marks, scans=scans)


def t2_want(key, scan):
    """The oracle's (find_t2sin, corr) of one scan."""
    c = t2_case(key)
    _, name, n, start = scan
    x = c["streams"][name]
    return O.find_t2sin(c["cfg"], x[:n], start), O.t2_corr(c["cfg"], x[start:n])


def t2_ratios(cfg, x):
    """The detector ratio of every whole block of x (NaN where the total is 0 or not finite)."""
    T, sm = cfg["t2sin_size"], cfg["smooth"]
    k = np.arange(T)
    mask = np.zeros(T)
    for f in (cfg["t2_sin_f1"], cfg["t2_sin_f2"]):
        mask += (k >= max(0, f - sm)) & (k <= min(T - 1, f + sm))
    with np.errstate(all="ignore"):
        X = np.fft.fft(x[:len(x) // T * T].reshape(-1, T), axis=1)
        e = X.real ** 2 + X.imag ** 2
        tot = e.sum(axis=1)
        return np.where(np.isfinite(tot) & (tot > 0), (e * mask).sum(axis=1) / tot, np.nan)


# ------------------------------------------------------------------ preamble cases
PRE_PAIRS = ((8, 64), (13, 64), (100, 128), (128, 256), (257, 512), (640, 1024), (640, 2048))  # (L, T2sin_size)
PRE_TEXTURES = ("f64", "capture", "weak")
PRE_SEEDS = {p: 900 + i for i, p in enumerate(PRE_PAIRS)}
PRE_THREADS = 256  # find_preamble_kernel: lags per slice
PRE_CORR_TAGS = ("lead", "hit2-5")  # the starts preamble_corr is checked at, per stream
NEAR_PAIRS = ((13, 64), (128, 256), (257, 512))
NEAR_D = (1e-9, 1e-11, 1e-13)


def pre_config(pair):
    L, T = pair
    return t2_config(T, pr_sin_len=L)


def pre_cycles(pair):
    return 2 * pair[1] + pair[0]


def pre_slices(pair):
    return -(-pre_cycles(pair) // PRE_THREADS)


def pre_lds_bytes(pair, split=True):
    """launch_find_preamble's dynamic LDS, by its own arithmetic."""
    L, C = pair[0], pre_cycles(pair)
    nn = C + L
    corr = 8 * C + 16 * ((min(C, PRE_THREADS) if split else C) + L)
    tail = 8 * (C + nn + nn + 1 + C + 16 + PRE_THREADS // 64) + 8 + 4 * ((C + 31) // 32) + 64
    return 16 + max(corr, tail)


@functools.lru_cache(maxsize=None)
def pre_template(pair):
    return O.preamble_setup(pre_config(pair))[2]


@functools.lru_cache(maxsize=None)
def pre_stream(pair, texture):
    """One (pair, texture) stream: dict(cfg, x, hits, starts [(tag, start)],
    cuts [(tag, n, start)], many: 100 starts). Textures: "f64" the impaired
    stream with a tail of noise alone; "capture" common.capture_stream (x mult,
    truncated to integers, exact-zero silences); "weak" the f64 stream scaled
    so that a window of noise alone holds an energy of about 0.1 and a window
    of signal about 10: the gate is closed over the gaps and open over the
    frames."""
    cfg = pre_config(pair)
    L, T = pair
    C = pre_cycles(pair)
    seed = PRE_SEEDS[pair]
    if texture == "capture":
        x = capture_stream(cfg, 3, seed, gap_max=2 * T)[0]
        marks = capture_marks(cfg, x)
    else:
        tail = C + L + 64
        # (a CFO of 0.3 / L at the most: 0.004 turns a 640-sample template 2.5 times and nothing correlates)
        x, marks = stream_with_marks(cfg, 3, seed, 2 * T, tail=tail, cfo_max=min(0.004, 0.3 / L))
        if texture == "weak":
            hit = marks[0]
            e_noise = float(np.mean(np.abs(x[-tail:]) ** 2))
            e_sig = float(np.mean(np.abs(x[hit + T: hit + T + O.geometry(cfg)["preamble_len"]]) ** 2))
            x = x / np.sqrt(L * np.sqrt(e_noise * e_sig))
    x = np.ascontiguousarray(x, np.complex128)
    n = len(x)
    hits = t2_hits(cfg, x, marks)
    h0, h1 = hits[0], hits[1]
    g = O.geometry(cfg)
    starts = [("hit", h0), ("hit-5", h0 - 5), ("zero", 0), ("negative", -(L // 2)), ("past-n", n - 50),
              ("hit2", h1), ("hit2-5", h1 - 5), ("lead", h0 - L - 7),
              ("mid-message", h0 + T + g["preamble_len"] + 11), ("mid-preamble", h0 + 2 * T + L // 2),
              ("tail", n - (C + L + 32)), ("hit3", hits[2])]
    cuts = [("cut-found", h1 + 2 * T + L, h1), ("cut-lost", h1 + T // 2, h1 - 5)]
    rng = np.random.default_rng(seed + 7)
    many = np.concatenate([[s for _, s in starts], rng.integers(-L, n, 100 - len(starts))]).astype(np.int32)
    x.setflags(write=False)
    return dict(cfg=cfg, x=x, n=n, hits=hits, starts=starts, cuts=cuts, many=many)


def pre_want(pair, x, n, starts):
    cfg, tpl = pre_config(pair), pre_template(pair)
    return [O.find_preamble(cfg, x[:n], int(s), tpl) for s in starts]


def _serial_ratio(seg, tpl, lag):
    """The ratio at one lag by the serial recurrence (find_corr_ref's norm, bit for bit)."""
    L = len(tpl)
    en = (seg.real * seg.real + seg.imag * seg.imag).tolist()
    norm = 0.0
    for i in range(L):
        norm += en[i]
    for i in range(lag):
        norm += en[i + L]
        norm -= en[i]
    return abs(complex(seg[lag: lag + L] @ tpl)) / np.sqrt(norm) if norm > 1.0 else 0.0


@functools.lru_cache(maxsize=None)
def near_level_cases(pair):
    """Streams whose first passing lag has a ratio of level (1 + d) or level
    (1 - d), d in NEAR_D: the f64 stream of the pair, searched from the second
    frame's T2 hit; the last L/2 samples of the first passing lag's window are
    scaled by a gain found by bisection (then a walk over neighbouring doubles)
    so that the ratio there, by the serial FP64 recurrence, is the target.
    List of dicts (d, sign, x, start, lag, ratio, achieved, want), the + and -
    case of each d adjacent."""
    base = pre_stream(pair, "f64")
    cfg, x0, n = base["cfg"], base["x"], base["n"]
    L, C = pair[0], pre_cycles(pair)
    tpl = pre_template(pair)
    level = cfg["pr_level"] / 1000
    start = base["hits"][1]
    cor, _ = find_corr_ref(x0, n, start, tpl, C)
    lag = int(np.nonzero(cor > level)[0][0])
    k = max(1, L // 2)
    lo, hi = start + lag + L - k, start + lag + L
    seg0 = np.array(x0[start: start + lag + L])

    def ratio(gain):
        seg = seg0.copy()
        seg[lo - start: hi - start] *= gain
        return _serial_ratio(seg, tpl, lag)

    assert ratio(1.0) > level > ratio(-1.0)
    out = []
    for d in NEAR_D:
        for sign in (1, -1):
            target = level * (1 + sign * d)
            a, b = -1.0, 1.0  # ratio(a) < target < ratio(b)
            for _ in range(70):
                mid = 0.5 * (a + b)
                if ratio(mid) < target:
                    a = mid
                else:
                    b = mid
            gain, best = b, np.inf
            for toward in (2.0, -2.0):  # the doubles around the root: the one nearest the target
                cand = b
                for _ in range(200):
                    miss = abs((ratio(cand) / level - 1) / (sign * d) - 1)
                    if miss < best:
                        gain, best = cand, miss
                    if best < 0.01:
                        break
                    cand = np.nextafter(cand, toward)
            x = np.array(x0)
            x[lo:hi] *= gain
            full, _ = find_corr_ref(x, n, start, tpl, C)
            x.setflags(write=False)
            out.append(dict(d=d, sign=sign, x=x, n=n, start=start, lag=lag, ratio=float(full[lag]),
                            achieved=float(full[lag] / level - 1), want=O.find_preamble(cfg, x, start, tpl)))
    return out


# ------------------------------------------------------------------ CFO cases
_CFO_DP = {64: (32, 4), 128: (64, 4), 256: (128, 8), 512: (256, 8), 1024: (512, 16), 2048: (1024, 32),
           4096: (2048, 64)}  # fft_size: (num_data_subc, num_pilot_subc)
# (fft_size, cp_size, nsym): one form per cfo_kernel instance, then the multi-symbol forms
CFO_FORMS = tuple([(n, 0, 1) for n in (64, 128, 256, 512, 1024, 2048, 4096)] +
                  [(n, n // 4, 1) for n in (256, 512, 1024, 2048, 4096)] +
                  [(64, 0, 2), (64, 16, 4), (128, 32, 4), (256, 64, 2), (512, 0, 8)])
CFO_INSTANCES = {(m, 1) for m in range(6, 13)} | {(m, 5) for m in range(6, 11)}
CFO_MULT = (-1.2, -0.4, 0.45, 1.2)  # the frames' CFO in units of 1 / fft_size (+- 0.05 of jitter)


def cfo_config(n, cp, nsym=1):
    d, p = _CFO_DP[n]
    return mkcfg(D, fft_size=n, cp_size=cp, num_data_subc=d, num_pilot_subc=p, num_symb=2, num_pr_symb=nsym,
                 pr_sin_len=min(128, n + cp))


def cfo_instance(form):
    """(logm, g) of a form as cfo_plan decides it: S = 2^logm, or 5 * 2^logm."""
    n, cp, nsym = form
    s = (n + cp) * nsym
    if s & (s - 1) == 0 and 6 <= s.bit_length() - 1 <= 12:
        return s.bit_length() - 1, 1
    q = s // 5
    assert s % 5 == 0 and q & (q - 1) == 0 and 6 <= q.bit_length() - 1 <= 10, form
    return q.bit_length() - 1, 5


def cfo_borders(form):
    """pilot_freq_sinh's window borders (P + 2 of them), as the oracle computes them."""
    n, cp, nsym = form
    d, p = _CFO_DP[n]
    size = (n + cp) * nsym
    rel_bw = (d + p) / n
    rel_pilot_w = rel_bw / p
    pilot_w = int(size * rel_pilot_w)
    b = [int((1.0 - rel_bw - rel_pilot_w) / 2.0 * size) + i * pilot_w for i in range(p + 2)]
    b[0] = max(0, b[0])
    return b


@functools.lru_cache(maxsize=None)
def cfo_case(form):
    """One form's frames: dict(cfg (num_pr_symb = nsym: the oracle's), S,
    stride, instance, x (6 frames at `stride`: 4 impaired, all zeros, a unit
    impulse at sample 0), kinds, want (the oracle's estimates))."""
    n, cp, nsym = form
    cfg = cfo_config(n, cp, nsym)
    S = (n + cp) * nsym
    stride = S + 37
    seed = 1100 + CFO_FORMS.index(form)
    rng = np.random.default_rng(seed)
    pre = O.preamble_setup(cfg)[0]
    assert len(pre) == S
    kinds = ["impaired"] * 4 + ["zeros", "impulse"]
    x = np.zeros(len(kinds) * stride, np.complex128)
    i = np.arange(S)
    for f, mult in enumerate(CFO_MULT):
        cfo = (mult + rng.uniform(-0.05, 0.05)) / n
        fr = pre * np.exp(2j * np.pi * cfo * i + 1j * rng.uniform(-np.pi, np.pi))
        x[f * stride: f * stride + S] = O.awgn(fr, 0.05, seed=seed * 10 + f)
    x[5 * stride] = 1.0
    want = np.array([O.pilot_freq_sinh(cfg, x[f * stride: f * stride + S]) for f in range(len(kinds))])
    x.setflags(write=False)
    return dict(cfg=cfg, S=S, stride=stride, instance=cfo_instance(form), x=x, kinds=kinds, want=want)


def cfo_window_gaps(form, fr):
    """Per window of one frame: (largest - second largest) / largest magnitude."""
    amp = np.fft.fftshift(np.abs(np.fft.fft(fr)))
    b = cfo_borders(form)
    p = len(b) - 2
    gaps = []
    for i in range(p + 1):
        if i == p // 2 or b[i + 1] - b[i] < 2:
            continue
        w = np.sort(amp[b[i]: b[i + 1]])
        gaps.append((w[-1] - w[-2]) / w[-1])
    return np.array(gaps)
