"""Streams that drive the stream walker's T2 decision through the zone its
FP32 screen's margin protects (tests/test_gpu_t2_near_level.py; the fixtures
themselves are checked on the CPU in tests/test_t2_level_cases.py).

Layout, on the block grid from sample 0 (the continuous walk, ring 0): `slot`
background blocks, one crafted block, 2 t2sin_size + 37 background samples,
then two ordinary frames with zero gaps. The crafted block is a tone(f1) plus
off-mask energy (a tone at the bin next to the mask edge, or white noise) with
the tone's amplitude solved so that the detector ratio is level + delta.
Nothing after the crafted block looks like a preamble: if the block passes,
the walk finds none, jumps message_len ahead and loses the first frame; if it
fails, both frames are found. The located frames reveal the decision.

The background is zeros, or weak white noise. Zeros are what a capture's
silence is, but a zero block is "uncertain" to the FP32 screen (total 0), so a
scan step that holds one before a block that is not a certain FAIL is decided
in FP64. With noise (a certain FAIL, ratio ~ the mask's share of the bins) the
crafted block's own FP32 verdict is the one the walk acts on."""
import numpy as np

import devtest as dt
import oracle as O

D = O.DEFAULT
CFG512 = dict(D, t2sin_size=512, t2_sin_f1=34, t2_sin_f2=102)
CONFIGS = {"t2sin256": (D, 4), "t2sin512": (CFG512, 2)}  # (config, G): the FP32 scan step screens 2 G blocks
MARGIN = 4e-5
MAGS = (0.25, 0.75, 1.25, 2.0, 8.0)  # |delta| / MARGIN
TEXTURES = ("edge", "white")
SCALES = (1e-3, 200.0, "int16")
FILLS = ("zeros", "noise")


def mask_of(cfg):
    n, sm = cfg["t2sin_size"], cfg["smooth"]
    f1, f2 = cfg["t2_sin_f1"], cfg["t2_sin_f2"]
    return (max(0, f1 - sm), min(n - 1, f1 + sm), max(0, f2 - sm), min(n - 1, f2 + sm))


def level_of(cfg):
    return cfg["t2_sin_level"] / 1000


def _tone(n, b):
    j = np.arange(n)
    return np.exp(2j * np.pi * ((b * j) % n) / n)


def crafted_block(cfg, delta, texture, scale, rng):
    """a tone(f1) + off-mask energy with detector ratio level + delta. The
    amplitude a from the closed form of the ratio (bins of exact tones are
    orthogonal; for white noise w the tone adds a n to w's bin f1); int16:
    rounded to integers at about 3e4 peak, the target moved by what the
    rounding shifted the longdouble ratio (a few 1e-7) and rounded again."""
    n, f1 = cfg["t2sin_size"], cfg["t2_sin_f1"]
    goal = level_of(cfg) + delta
    if texture == "edge":
        off = _tone(n, f1 + cfg["smooth"] + 1)
    else:
        off = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2 * n)
        W = np.fft.fft(off)
        e = np.abs(W) ** 2
        em, et = float(np.sum(dt.t2_mask(n, mask_of(cfg)) * e)), float(np.sum(e))

    peak = []  # int16: the scale is fixed by the first solution, so the block moves little with r

    def block(r):
        if texture == "edge":
            a = np.sqrt(r / (1 - r))
        else:
            A = (r * et - em) / (1 - r)  # a^2 n^2 + 2 a n Re W[f1]
            a = (-W[f1].real + np.sqrt(W[f1].real ** 2 + A)) / n
        x = a * _tone(n, f1) + off
        if scale != "int16":
            return x * scale
        if not peak:
            peak.append(30000.0 / max(np.abs(x.real).max(), np.abs(x.imag).max()))
        x = x * peak[0]
        return np.round(x.real) + 1j * np.round(x.imag)

    x = block(goal)
    if scale == "int16":
        r = goal
        for _ in range(6):
            r += goal - float(dt.t2_ratio_ref(x[None, :], mask_of(cfg))[0])
            x = block(r)
    return x


_frames = {}


def _two_frames(key, cfg, int16):
    k = (key, int16)
    if k not in _frames:
        g = O.geometry(cfg)
        data = np.random.default_rng(99).integers(0, 256, 2 * g["bytes_per_frame"], dtype=np.uint8)
        fr = [O.frame_write(cfg, data[i * g["bytes_per_frame"]:(i + 1) * g["bytes_per_frame"]]) for i in (0, 1)]
        if int16:
            fr = [O.get_int16(f, cfg["mult"]).astype(np.float64) for f in fr]
            fr = [f[0::2] + 1j * f[1::2] for f in fr]
        _frames[k] = fr
    return _frames[k]


def build_stream(key, case, rng):
    """The stream of one case and its crafted block: (x complex128, block)."""
    cfg, _ = CONFIGS[key]
    n = cfg["t2sin_size"]
    int16 = case["scale"] == "int16"
    block = crafted_block(cfg, case["delta"], case["texture"], case["scale"], rng)
    head = (case["slot"] + 1) * n + 2 * n + 37
    if case["fill"] == "zeros":
        bg = np.zeros(head, np.complex128)
    elif int16:  # a few counts of white noise
        bg = rng.integers(-3, 4, head) + 1j * rng.integers(-3, 4, head)
    else:
        s = float(np.sqrt(np.mean(np.abs(block) ** 2))) * 1e-3
        bg = (rng.standard_normal(head) + 1j * rng.standard_normal(head)) * s
    bg[case["slot"] * n:(case["slot"] + 1) * n] = block
    f0, f1 = _two_frames(key, cfg, int16)
    z = np.zeros
    x = np.concatenate([bg, f0, z(333, np.complex128), f1, z(O.geometry(cfg)["frame_len"], np.complex128)])
    return np.ascontiguousarray(x, np.complex128), block


_cases = {}


def cases(key):
    """Every case of one config, as +delta / -delta pairs that share all else:
    list of dicts (delta, mag, slot, texture, scale, fill, x, block, ratio:
    the block's longdouble detector ratio, want: the oracle's walk). Every
    |delta| with every slot (the 2 G blocks of the first scan step and two of
    the second, one per packed lane); texture, scale and background cycle
    along the list."""
    if key in _cases:
        return _cases[key]
    cfg, G = CONFIGS[key]
    slots = list(range(2 * G)) + [2 * G + 1, 3 * G]
    out, i = [], 0
    for slot in slots:
        for mag in MAGS:
            common = dict(mag=mag, slot=slot, texture=TEXTURES[i % 2], scale=SCALES[(i // 2) % 3],
                          fill=FILLS[(i // 6 + i) % 2])
            for sign in (1, -1):
                c = dict(common, delta=sign * mag * MARGIN, pair=i)
                # the two signs share the noise: the same seed
                c["x"], c["block"] = build_stream(key, c, np.random.default_rng(5000 + i))
                out.append(c)
            i += 1
    ratios = dt.t2_ratio_ref(np.stack([c["block"] for c in out]), mask_of(cfg))
    for c, r in zip(out, ratios):
        c["ratio"] = r
        c["want"] = O.stream_walk(cfg, c["x"])
        c["x"].setflags(write=False)
    _cases[key] = out
    return out


def int16_wire(x):
    """The interleaved complex<int16> samples of an integer-valued stream."""
    w = np.empty(2 * len(x), np.int16)
    w[0::2], w[1::2] = x.real.astype(np.int16), x.imag.astype(np.int16)
    return w
