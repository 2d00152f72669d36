"""Shared test helpers: golden fixtures, configs, seeded payloads."""
import json
import os

import numpy as np

import oracle as O

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    with open(os.path.join(GOLDEN_DIR, "golden.json")) as f:
        meta = json.load(f)
    g = dict(meta)
    g["source"] = np.load(os.path.join(GOLDEN_DIR, "source_bin.npy"))
    g["data_i16"] = np.load(os.path.join(GOLDEN_DIR, "data_bin_i16.npz"))["iq"]  # interleaved complex<int16>
    d = g["data_i16"].astype(np.float64)
    g["data"] = d[0::2] + 1j * d[1::2]
    g["t2_corr"] = np.load(os.path.join(GOLDEN_DIR, "t2_sin_corr.npy"))
    g["phases"] = np.load(os.path.join(GOLDEN_DIR, "phases.npy"))
    g["constell"] = np.load(os.path.join(GOLDEN_DIR, "constell.npy"))
    with open(os.path.join(GOLDEN_DIR, "data_txt.bin"), "rb") as f:
        g["payload_text"] = np.frombuffer(f.read(), np.uint8)
    g["payload"] = np.concatenate([np.array(meta["mac_header"], np.uint8), g["payload_text"]])
    return g


def payload(nbytes: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def cfg(base: dict, **kw) -> dict:
    d = dict(base)
    d.update(kw)
    return d


# Configs used across tests (D default, G golden, B 2048/QPSK, C 4096/16-QAM)
D = O.DEFAULT
G = O.GOLDEN
B = O.CONFIG_B
CC = O.CONFIG_C
EXTRA = {
    "D_qam64": cfg(O.DEFAULT, mod_type=6),
    "D_qam256": cfg(O.DEFAULT, mod_type=8),
    "D_qpsk": cfg(O.DEFAULT, mod_type=2),
    "N1024_k4": cfg(O.DEFAULT, fft_size=1024, num_data_subc=512, num_pilot_subc=16, cp_size=256),
    "N256_k2": cfg(O.DEFAULT, fft_size=256, num_data_subc=128, num_pilot_subc=8, cp_size=64, mod_type=2),
    "N128_k4_s3": cfg(O.DEFAULT, fft_size=128, num_data_subc=64, num_pilot_subc=4, cp_size=16, num_symb=3),
    "N64_k1": cfg(O.DEFAULT, fft_size=64, num_data_subc=32, num_pilot_subc=4, cp_size=16, mod_type=1,
                  num_symb=2, pr_sin_len=64, t2sin_size=64, t2_sin_f1=5, t2_sin_f2=20, smooth=2),
    "D_s12_staged": cfg(O.DEFAULT, num_symb=12),
    "D_s1": cfg(O.DEFAULT, num_symb=1),
    "D_p2": cfg(O.DEFAULT, num_pilot_subc=2),
    "D_cp0": cfg(O.DEFAULT, cp_size=0),
    "D_p16": cfg(O.DEFAULT, num_pilot_subc=16),  # S*P = 128 > 64: rx_wide_kernel's phys broadcast
}
ALL_CONFIGS = {"D": D, "G": G, "B": B, "C": CC, **EXTRA}


def rel_err(a, b) -> float:
    a = np.asarray(a)
    b = np.asarray(b)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def assert_int16_match(got16, ref_iq, mult):
    """int16 wire samples (FRAME_FORM::get_int16 = trunc(x*mult)) must be
    identical, except where x*mult lies within 1e-9 of an integer: there the
    truncation is decided by FFT rounding order (FFTW, oracle and GPU all
    differ in the last ulp) and a 1-LSB difference is allowed."""
    v = np.empty(2 * ref_iq.size)
    v[0::2] = ref_iq.real.ravel() * mult
    v[1::2] = ref_iq.imag.ravel() * mult
    got = got16.ravel().astype(np.int64)
    want = np.trunc(v).astype(np.int64)
    diff = got != want
    ambiguous = np.abs(v - np.round(v)) < 1e-9 * np.maximum(1.0, np.abs(v))
    assert np.all(ambiguous[diff]), f"{int((diff & ~ambiguous).sum())} non-ambiguous int16 mismatches"
    assert np.all(np.abs(got - want)[diff] <= 1)
    return int(diff.sum())


def impaired_stream(cfg, nf, seed, snr_db=20.0, cfo_max=0.004, gap_max=4096):
    """Config-4 stream: full frames (T2+preamble+message) with random 0..gap_max
    zero gaps, per-frame CFO U(-cfo_max, cfo_max) and phase, AWGN over all."""
    g = O.geometry(cfg)
    rng = np.random.default_rng(seed)
    data = payload(nf * g["bytes_per_frame"], seed)
    parts = [np.zeros(int(rng.integers(0, gap_max + 1)), np.complex128)]
    for f in range(nf):
        fr = O.frame_write(cfg, data[f * g["bytes_per_frame"]:(f + 1) * g["bytes_per_frame"]])
        n = np.arange(len(fr))
        fr = fr * np.exp(2j * np.pi * rng.uniform(-cfo_max, cfo_max) * n + 1j * rng.uniform(-np.pi, np.pi))
        parts += [fr, np.zeros(int(rng.integers(0, gap_max + 1)), np.complex128)]
    x = np.concatenate(parts)
    return O.awgn(x, 10 ** (-snr_db / 20), seed=seed), data


def capture_stream(cfg, nf, seed, gap_max=3000):
    """A wire capture as tx.cpp + the SDR stand-in make it (data/tx.bin
    layout): full frames in FRAME_FORM::get_int16 scaling (x mult), exact-zero
    silences of 0..gap_max samples between them (no noise), one frame_len of
    zeros at the end. Returns (complex128 samples, interleaved int16)."""
    g = O.geometry(cfg)
    rng = np.random.default_rng(seed)
    data = payload(nf * g["bytes_per_frame"], seed)
    parts = []
    for f in range(nf):
        fr = O.frame_write(cfg, data[f * g["bytes_per_frame"]:(f + 1) * g["bytes_per_frame"]])
        parts += [np.zeros((int(rng.integers(0, gap_max + 1)), 2), np.int16),
                  O.get_int16(fr, cfg["mult"]).reshape(-1, 2)]
    parts.append(np.zeros((g["frame_len"], 2), np.int16))
    x16 = np.ascontiguousarray(np.concatenate(parts).reshape(-1))
    w = x16.astype(np.float64)
    return w[0::2] + 1j * w[1::2], x16


def decision_thresholds(k):
    """Modulation::demod's cell edges on each axis (modulation.cpp:53-87)."""
    m = 1 << (k // 2)
    s1 = (m - 1) / 2.0
    return np.array([(j - 0.5) / s1 - 1.0 for j in range(1, m)])


def distance_to_threshold(k, pts):
    """Distance of each equalised point from the decision edge nearest to it
    (BPSK: the line re + im = 0; QAM: the clamped re / im cell edges)."""
    if k == 1:
        return np.abs(pts.real + pts.imag)
    th = decision_thresholds(k)
    dre = np.min(np.abs(np.clip(pts.real, -1, 1)[..., None] - th), axis=-1)
    dim = np.min(np.abs(np.clip(pts.imag, -1, 1)[..., None] - th), axis=-1)
    return np.minimum(dre, dim)


def check_stream_frames(cfg, x, pbs, got_bytes, got_cons, got_cfo=None, tol=1e-9, allow_flips=False, threads=0):
    """Every located frame of a stream against the oracle's main.cpp:60-80
    chain on the same samples (orc_decode_frames): CFO exact, constellation
    within `tol` relative per frame, and every byte equal, except that a
    decision may differ where the oracle's own point lies within the rounding
    band of its threshold (twice the largest GPU-oracle point difference of
    the whole stream: the sync chain's transcendentals and the FFT round
    differently). With allow_flips False (the default) no
    decision may differ at all: north_star's bit-exact decisions. `threads`:
    the oracle's decode threads (0 = one per CPU; a test that checks many
    short streams passes a small number). Returns a summary dict."""
    k = cfg["mod_type"]
    g = O.geometry(cfg)
    nf = len(pbs)
    ocfo, ocons, obytes = O.decode_frames(cfg, x, pbs, threads=threads)
    if got_cfo is not None:
        bad = np.nonzero(got_cfo != ocfo)[0]
        assert bad.size == 0, f"CFO differs on {bad.size} frames, first {bad[:8]}"
    scale = np.abs(ocons).max(axis=1)
    err = np.abs(got_cons - ocons).max(axis=1) / np.maximum(scale, 1e-300)
    assert err.max() < tol, f"constellation rel err {err.max():.2e} on frame {int(err.argmax())}"
    band = 2.0 * float(np.abs(got_cons - ocons).max())
    diff_frames = np.nonzero(np.any(got_bytes != obytes, axis=1))[0]
    flips, worst = 0, 0.0
    for f in diff_frames:
        bg = np.unpackbits(got_bytes[f])[:g["npts"] * k].reshape(-1, k)
        bo = np.unpackbits(obytes[f])[:g["npts"] * k].reshape(-1, k)
        pts = np.nonzero(np.any(bg != bo, axis=1))[0]
        d = distance_to_threshold(k, ocons[f][pts])
        flips += len(pts)
        worst = max(worst, float(d.max()))
        assert np.all(d <= band), (f"frame {f}: {len(pts)} decisions differ, farthest {d.max():.3e} "
                                   f"from its threshold (band {band:.3e})")
    assert allow_flips or flips == 0, f"{flips} decisions differ from the oracle on {diff_frames.size} frames"
    return {"frames": nf, "max_constellation_rel_err": float(err.max()), "band": band,
            "frames_with_flips": int(diff_frames.size), "decision_flips": flips,
            "farthest_flip_from_threshold": worst}


# ------------------------------------------------------------ non-flat channels
# Frames whose channel estimate has work to do: a multipath channel, or a
# region cut a few samples early (inside the cyclic prefix), turns
# chan_char_lq's per-carrier phases into a ramp that wraps, so its one-pass
# unwrap adjusts tens to hundreds of entries where a flat channel at the exact
# start adjusts none.
def _apply_taps(x, taps):
    """y[n] = sum_k gain_k x[n - delay_k], cut to len(x)."""
    y = np.zeros(len(x), np.complex128)
    for delay, gain in taps:
        y[delay:] += complex(gain) * x[: len(x) - delay]
    return y


def channel_frames(cfg, nf, seed, taps=((0, 1.0),), offset=0, snr_db=34.0, cfo_max=0.002):
    """[preamble | message] regions of nf oracle-written frames, each frame
    convolved with `taps` (a list of (delay, complex gain)), given a CFO
    U(-cfo_max, cfo_max) and a constant phase, AWGN `snr_db` below the
    frame's rms (34 dB: 0.02 rms), and cut `offset` samples before the true
    preamble start (0 <= offset <= t2sin_size). Returns (regions (nf, n), data)."""
    g = O.geometry(cfg)
    t2, n = cfg["t2sin_size"], g["preamble_len"] + g["message_len"]
    assert 0 <= offset <= t2
    rng = np.random.default_rng(seed)
    data = payload(nf * g["bytes_per_frame"], seed)
    out = np.zeros((nf, n), np.complex128)
    for f in range(nf):
        fr = O.frame_write(cfg, data[f * g["bytes_per_frame"]:(f + 1) * g["bytes_per_frame"]])
        fr = _apply_taps(fr, taps)
        i = np.arange(len(fr))
        fr = fr * np.exp(2j * np.pi * rng.uniform(-cfo_max, cfo_max) * i + 1j * rng.uniform(-np.pi, np.pi))
        rms = float(np.sqrt(np.mean(np.abs(fr) ** 2)))
        fr = O.awgn(fr, rms * 10 ** (-snr_db / 20), seed=seed * 100 + f)
        out[f] = fr[t2 - offset: t2 - offset + n]
    return out, data


def channel_stream(cfg, nf, seed, taps=((0, 1.0),), snr_db=34.0, cfo_max=0.004, gap_max=4096):
    """impaired_stream through a channel: full frames with random 0..gap_max
    zero gaps, per-frame CFO and phase, `taps` applied over the concatenation,
    AWGN `snr_db` below the frames' rms over all. Returns (samples, data)."""
    g = O.geometry(cfg)
    rng = np.random.default_rng(seed)
    data = payload(nf * g["bytes_per_frame"], seed)
    parts = [np.zeros(int(rng.integers(0, gap_max + 1)), np.complex128)]
    power = 0.0
    for f in range(nf):
        fr = O.frame_write(cfg, data[f * g["bytes_per_frame"]:(f + 1) * g["bytes_per_frame"]])
        i = np.arange(len(fr))
        fr = fr * np.exp(2j * np.pi * rng.uniform(-cfo_max, cfo_max) * i + 1j * rng.uniform(-np.pi, np.pi))
        power += float(np.mean(np.abs(fr) ** 2)) / nf
        parts += [fr, np.zeros(int(rng.integers(0, gap_max + 1)), np.complex128)]
    x = _apply_taps(np.concatenate(parts), taps)
    return O.awgn(x, np.sqrt(power) * 10 ** (-snr_db / 20), seed=seed), data


def chan_phase_path(cfg, pre_region, mod_preamble=None):
    """chan_char_lq's phase path restated in numpy (from oracle/ofdm_oracle.c,
    orc_chan_char_lq): the raw phases of the first D/2 carriers of the synced
    preamble over the preamble's own BPSK points, the serial one-pass unwrap
    (an entry moves by -/+2 pi when it differs from the already adjusted
    previous one by more than pi), the line through (i, phase) from raw sums,
    and the unit phasors over the D carriers. Returns a dict:
    raw, unwrapped, adjust (per entry -1/0/+1: the scan's state minus 1),
    adjusted (count), state_changes, pi_margin (the least distance of any
    compare from +-pi, over all three states the previous entry could be in),
    a, b, chan."""
    D = cfg["num_data_subc"]
    half = D // 2
    if mod_preamble is None:
        mod_preamble = O.preamble_setup(cfg)[1]
    pr = O.ofdm_fft(cfg, np.asarray(pre_region)[: O.geometry(cfg)["preamble_len"]], S=cfg["num_pr_symb"])
    q = pr[:half] / np.asarray(mod_preamble)[:half]
    raw = np.arctan2(q.imag, q.real)
    two_pi = 2 * np.pi
    ph = raw.copy()
    adjust = np.zeros(half, np.int64)
    margin = np.inf
    for i in range(1, half):
        for k in (-1, 0, 1):  # the compare in each state of entry i - 1
            d = raw[i] - (raw[i - 1] + k * two_pi)
            margin = min(margin, abs(d - np.pi), abs(d + np.pi))
        d = ph[i] - ph[i - 1]
        if d > np.pi:
            ph[i] -= two_pi
            adjust[i] = -1
        elif d < -np.pi:
            ph[i] += two_pi
            adjust[i] = 1
    mx = my = mxy = mx2 = 0.0
    for i in range(half):
        mxy += ph[i] * i
        mx2 += i * i
        mx += i
        my += ph[i]
    b = (mxy - mx * my) / (mx2 - mx * mx)  # raw sums, not means: as the reference has it
    a = my - b * mx
    i = np.arange(D)
    arg = np.where(i < D // 2, b * i + a, -b * D / 2 + (i - D // 2) * b + a)
    return {"raw": raw, "unwrapped": ph, "adjust": adjust, "adjusted": int(np.count_nonzero(adjust)),
            "state_changes": int(np.count_nonzero(np.diff(adjust))), "pi_margin": float(margin),
            "a": a, "b": b, "chan": np.exp(1j * arg)}


def synced_region(cfg, region):
    """main.cpp:60-64 on one [preamble | message] region in the oracle:
    (cfo, the region after freq_shift, cp_freq_sinh and pr_phase_sinh)."""
    g = O.geometry(cfg)
    pre = O.preamble_setup(cfg)[0]
    cfo = O.pilot_freq_sinh(cfg, region[: g["preamble_len"]])
    return cfo, O.pr_phase_sinh(O.cp_freq_sinh(cfg, O.freq_shift(region, cfo)), pre)


TAPS_FLAT = [(0, 1.0)]
TAPS_ECHO = [(0, 1.0), (3, 0.5j)]
TAPS_NOTCH = [(0, 1.0), (1, -0.9)]
TAPS_LATE = [(0, 0.5), (7, 1.0)]  # the later tap is the stronger
D384 = cfg(D, num_data_subc=384)  # half = 192: 3 entries per thread in chan_kernel's unwrap (T = 64)
D448 = cfg(D, num_data_subc=448)  # half = 224: 4 entries per thread

# (name, config, taps, offset, seed, frames): the frames of the GPU sync tests
# (tests/test_gpu_channel.py). tests/test_channel_cases.py asserts on the CPU
# that each one is well conditioned and makes the unwrap work.
CHANNEL_CASES = [
    ("N64_k1-flat-o5", EXTRA["N64_k1"], TAPS_FLAT, 5, 31, 4),
    ("N64_k1-notch-o2", EXTRA["N64_k1"], TAPS_NOTCH, 2, 32, 4),
    ("N128_k4_s3-echo-o5", EXTRA["N128_k4_s3"], TAPS_ECHO, 5, 33, 4),
    ("D-notch-o17", D, TAPS_NOTCH, 17, 34, 4),
    ("D-echo-o64", D, TAPS_ECHO, 64, 35, 3),
    ("N1024_k4-echo-o17", EXTRA["N1024_k4"], TAPS_ECHO, 17, 36, 3),
    ("B-flat-ocp2", B, TAPS_FLAT, B["cp_size"] // 2, 37, 3),
    ("B-notch-o5", B, TAPS_NOTCH, 5, 38, 3),
    ("C-echo-o17", CC, TAPS_ECHO, 17, 39, 3),
]
# chan_estimate alone accepts these (rx refuses D > N/2)
CHAN_ONLY_CASES = [
    ("D384-flat-o64", D384, TAPS_FLAT, 64, 41, 3),
    ("D384-notch-o17", D384, TAPS_NOTCH, 17, 42, 3),
    ("D448-echo-o64", D448, TAPS_ECHO, 64, 43, 3),
    ("D448-notch-o5", D448, TAPS_NOTCH, 5, 44, 3),
]
N1024_WIDE = cfg(B, fft_size=1024, num_data_subc=512, num_pilot_subc=16, cp_size=256)
TAPS_LATE3 = [(0, 0.9j), (3, 1.0)]
TAPS_LATE20 = [(0, 0.8), (20, 1.0)]
TAPS_THREE = [(0, 0.6), (5, 1.0), (9, -0.5j)]
# (name, config, taps, seed, frames, format): the streams of the non-flat
# stream tests (tests/test_gpu_stream.py). The detector chooses each frame's
# offset there: with a later tap the stronger it fires on the early one, and
# the region starts before the bulk of the energy.
STREAM_CASES = [
    ("stream-D-late3", D, TAPS_LATE3, 61, 8, "f64"),
    ("stream-D-late7", D, TAPS_LATE, 62, 8, "f64"),
    ("stream-D-three-i16", D, TAPS_THREE, 61, 8, "i16"),
    ("stream-D_s12-three", EXTRA["D_s12_staged"], TAPS_THREE, 61, 8, "f64"),
    ("stream-B-late20", B, TAPS_LATE20, 62, 8, "f64"),
    ("stream-B-late3-i16", B, TAPS_LATE3, 61, 8, "i16"),
    ("stream-N1024-late20", N1024_WIDE, TAPS_LATE20, 62, 8, "f64"),
]
STREAM_CASE = {c[0]: c for c in STREAM_CASES}


def stream_case_samples(case):
    """The samples of one STREAM_CASES entry: (complex128 samples, interleaved
    int16 or None). An "i16" stream is scaled and truncated as the wire format
    is (FRAME_FORM::get_int16, x mult, as capture_stream does), and its
    complex128 samples are those integers."""
    name, c, taps, seed, nf, fmt = case
    x, _ = channel_stream(c, nf, seed, taps)
    if fmt == "f64":
        return x, None
    x16 = O.get_int16(x, c["mult"])
    w = x16.astype(np.float64)
    return w[0::2] + 1j * w[1::2], x16
