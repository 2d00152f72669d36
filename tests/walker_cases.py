"""Fixtures of the stream receiver's geometry tests
(tests/test_gpu_walker_geometry.py: ofdm_rx_stream / ofdm_rx_stream_i16 on
every stream_walk_kernel instance, both preamble searches at window counts 1
to 72, and the decode kernels no other stream test launches; the fixtures
themselves are checked on the CPU in tests/test_walker_cases.py). No torch, no
GPU: numpy and the oracle.

- WALKER: (T2sin_size, pr_sin_len) pairs over detector_cases.t2_config with
  rx_buf_size = 3 (a ring end every three frames), and what each aims at.
- DECODE: overrides of the default config whose located frames take the narrow
  fused decode (stream_decode_kernel) or the staged stream kernels at N = 64,
  128, 256 and 4096.
- expected_walker / walker_lds / expected_decode: WalkShape, WalkLds and the
  decode dispatch (fused_geometry, launch_stream_decode, rx_dispatch's stream
  branch) restated.
- streams: per case an impaired stream, its int16 form (x 200, rounded; the
  samples are those integers) and, per T2 size, a wire capture with exact-zero
  silences; and per walker case two one-frame streams whose first passing
  lag is among the preamble search's last lags, or just past them.
"""
import functools

import numpy as np

import oracle as O
from common import D, capture_stream, cfg as mkcfg, distance_to_threshold, impaired_stream
from detector_cases import T2_TONES, t2_config
from rx_geometry_cases import EDGE_BAR, LDS_LIMIT, RX_DPT, RX_SMAX  # noqa: F401  (EDGE_BAR: the tests' bar)

WALK_FFT_M = 512        # ofdm_sync.hpp: the FFT preamble search's transform
FFT_L_MAX = WALK_FFT_M - 63  # ofdm_create builds a template spectrum up to here: windows of >= 64 lags
I16_SCALE = 200.0       # the wire scaling of the int16 form (FRAME_FORM::get_int16's mult)
WALKER_SEED, DECODE_SEED = 31, 41
WALKER_FRAMES, DECODE_FRAMES, CAPTURE_FRAMES = 12, 10, 8

# (T2sin_size, pr_sin_len, what it reaches)
_WALKER = [
    (64, 64, "G = 16 screen; one window (Q = 449 >= C = 192)"),
    (64, 449, "G = 16; 10 windows of 64 lags, the last of 1"),
    (64, 640, "G = 16; the direct certified search"),
    (128, 128, "G = 8 screen; one window of 384 lags"),
    (128, 450, "G = 8; the first direct length"),
    (256, 300, "G = 4; 4 windows of 213 lags, the last of 173"),
    (256, 449, "G = 4; 16 windows, the last of 1 lag"),
    (256, 450, "G = 4; direct"),
    (512, 64, "G = 2 screen; 3 windows"),
    (512, 640, "G = 2; direct"),
    (1024, 128, "FP64-only scan, two waves per transform (NW = 2); 6 windows"),
    (1024, 449, "FP64-only scan; 40 windows"),
    (1024, 640, "FP64-only scan; direct"),
    (2048, 64, "the 256-thread walker (NW = 4); 10 windows"),
    (2048, 449, "256 threads; 72 windows: the largest walker LDS that fits"),
]
WALKER = {f"T{t}-L{length}": (t, length) for t, length, _ in _WALKER}
WALKER_AIMS = {f"T{t}-L{length}": aim for t, length, aim in _WALKER}
WALKER_NAMES = list(WALKER)
T2_SIZES = sorted({t for t, _ in WALKER.values()})

# configs the stream call refuses (walker_lds over the limit, or no walker at all)
REFUSED = {"T2048-L450": (2048, 450), "T2048-L640": (2048, 640), "T4096-L128": (4096, 128)}


def walker_config(size, length):
    return t2_config(size, rx_buf_size=3, pr_sin_len=length)


def _t2(size):
    f1, f2, sm = T2_TONES[size]
    return dict(t2sin_size=size, t2_sin_f1=f1, t2_sin_f2=f2, smooth=sm)


# (name, overrides of D, the decode path it is in the table for, note)
_DECODE = [
    ("fused-S1-P64", dict(num_symb=1, num_pilot_subc=64), ("fused-narrow",), "one symbol, P at the kernel's bound"),
    ("fused-S3-D64-P2-k6", dict(num_symb=3, num_data_subc=64, num_pilot_subc=2, mod_type=6), ("fused-narrow",),
     "odd S, D = T, two pilots, 64-QAM"),
    ("fused-S5-D200-P4-k8", dict(num_symb=5, num_data_subc=200, num_pilot_subc=4, mod_type=8), ("fused-narrow",),
     "D no multiple of 64, 256-QAM"),
    ("fused-S7-D8-P2-k2", dict(num_symb=7, num_data_subc=8, num_pilot_subc=2, mod_type=2), ("fused-narrow",),
     "D far below T"),
    ("fused-S8-D248-P62-k1", dict(num_symb=8, num_data_subc=248, num_pilot_subc=62, mod_type=1), ("fused-narrow",),
     "P near 64, BPSK"),
    ("N256-cp64", dict(fft_size=256, cp_size=64, num_data_subc=128, num_pilot_subc=8, mod_type=2, num_symb=3),
     ("staged", 8, (6, 5), "rx_kernel"), "cfo_kernel<6,5>"),
    ("N256-cp0", dict(fft_size=256, cp_size=0, num_data_subc=104, num_pilot_subc=4, mod_type=4, num_symb=5),
     ("staged", 8, (8, 1), "rx_kernel"), "cfo_kernel<8,1>"),
    ("N128-cp0", dict(fft_size=128, cp_size=0, num_data_subc=64, num_pilot_subc=4, num_symb=8, pr_sin_len=128,
                      **_t2(128)), ("staged", 7, (7, 1), "rx_kernel"), "cfo_kernel<7,1>"),
    ("N64-cp0", dict(fft_size=64, cp_size=0, num_data_subc=32, num_pilot_subc=4, mod_type=2, num_symb=8,
                     pr_sin_len=64, **_t2(64)), ("staged", 6, (6, 1), "rx_kernel"), "cfo_kernel<6,1>"),
    ("N4096-cp0", dict(fft_size=4096, cp_size=0, num_data_subc=2040, num_pilot_subc=204, mod_type=2, num_symb=2),
     ("staged", 12, (12, 1), "rx_kernel"), "cfo_kernel<12,1>, stream_params_kernel<12>"),
]
DECODE = {name: mkcfg(D, **kw) for name, kw, _, _ in _DECODE}
DECODE_MEANT = {name: meant for name, _, meant, _ in _DECODE}
DECODE_NOTES = {name: note for name, _, _, note in _DECODE}
DECODE_NAMES = list(DECODE)
FUSED_NAMES = [n for n in DECODE_NAMES if DECODE_MEANT[n] == ("fused-narrow",)]
# what staged_decode = 1 makes of a narrow-fused case
FUSED_STAGED = ("staged", 9, (7, 5), "rx_stream2")


# ------------------------------------------------------------------ the library's rules, restated
def expected_walker(c):
    """(logt, threads, G, fp32_screen, search, windows) of a config's walker:
    WalkShape (128 threads, or T2sin_size / 8 above 1024; G blocks per scan
    step), the FP32 T2 screen (transforms of one wave: T2sin_size <= 512), and
    the preamble search: "fft" in windows of Q = M + 1 - L lags over C = 2 T2 +
    L lags where ofdm_create builds a template spectrum (L <= M - 63), else
    "direct" (windows 0). A T2 size without a walker raises."""
    n, length = c["t2sin_size"], c["pr_sin_len"]
    logt = n.bit_length() - 1
    if n != 1 << logt or not 6 <= logt <= 11:
        raise ValueError("no walker")
    t = n // 8
    threads = max(t, 128)
    if length <= FFT_L_MAX:
        q, cyc = WALK_FFT_M + 1 - length, 2 * n + length
        return logt, threads, threads // t, t <= 64, "fft", -(-cyc // q)
    return logt, threads, threads // t, t <= 64, "direct", 0


def windows(c):
    """The lags of each window of the FFT search: nl = min(Q, C - i0)."""
    q, cyc = WALK_FFT_M + 1 - c["pr_sin_len"], 2 * c["t2sin_size"] + c["pr_sin_len"]
    return [min(q, cyc - i0) for i0 in range(0, cyc, q)]


def walker_lds(c):
    """The walker's dynamic LDS in bytes: WalkLds<LOGT>::FIXED + big(L, C, fft)."""
    logt, threads, g, _, search, _ = expected_walker(c)
    n, length = 1 << logt, c["pr_sin_len"]
    t, cyc, fft = n // 8, 2 * n + length, search == "fft"
    nw = t // 64 if t >= 64 else 1
    tw = lambda size: size // 64 + 64  # noqa: E731  TwLds::SIZE
    fixed = 16 * (tw(n) + g * nw) + 8 * 2 * (threads // 64) + 16 + 8 * 16 + 16 * tw(WALK_FFT_M)
    t2 = 16 * g * n
    fs = (16 + 8) * WALK_FFT_M if fft else 0
    ex = 16 * (cyc + length) + 8 * cyc
    di = 0 if fft else ex + 8 * (cyc + length) + 16 + 16 * length
    return fixed + max(t2, fs, ex, di)


def cfo_form(c):
    """(logm, g) of the preamble form's pilot_freq_sinh plan (cfo_plan), or None."""
    s = (c["fft_size"] + c["cp_size"]) * c["num_pr_symb"]
    if s & (s - 1) == 0 and 6 <= s.bit_length() - 1 <= 12:
        return s.bit_length() - 1, 1
    q = s // 5
    if s % 5 == 0 and q & (q - 1) == 0 and 6 <= q.bit_length() - 1 <= 10:
        return q.bit_length() - 1, 5
    return None


def fused_geometry(c):
    """fused_geometry (csrc/ofdm_stream_call.cpp): the decode kernels that read the frames in place."""
    n, cp, s = c["fft_size"], c["cp_size"], c["num_symb"]
    t, sym = n // 8, n + cp
    return (s <= RX_SMAX and c["num_data_subc"] <= RX_DPT * t and c["num_pilot_subc"] <= t and c["num_pr_symb"] == 1
            and sym % t == 0 and sym // t <= 16 and cp <= 2 * t and cfo_form(c) is not None)


def _wide_shm(c):
    n, s, p = c["fft_size"], c["num_symb"], c["num_pilot_subc"]
    logn, t = n.bit_length() - 1, n // 8
    m = n // 4
    end = 7 * n // 4 + (m // 64 + 64) + t + 32 + 16 + 32 + 32 + (t + 2 + 3) // 4
    region = (end + 7) // 8 * 8 if end > 2 * n else 2 * n
    rts = 8 + (logn - 6) + 1
    return 16 * ((n // 64 + 64) + region + s * p + max(s * p, rts * s) + 2)


def expected_decode(c, staged_decode=False):
    """The decode path of a config's located frames: ("gathered",),
    ("fused-wide", logn), ("fused-narrow",), or ("staged", logn, (logm, g) of
    the CFO kernel, "rx_stream2" | "rx_kernel"): decode_list, decode_fused,
    launch_stream_decode (stream_decode_wide_fits, stream_sync_geometry) and
    rx_dispatch's stream branch. staged_decode: the walk tuning of that name."""
    if not fused_geometry(c):
        return ("gathered",)
    n, cp, s, d, p = c["fft_size"], c["cp_size"], c["num_symb"], c["num_data_subc"], c["num_pilot_subc"]
    logn, t = n.bit_length() - 1, n // 8
    logm, g = cfo_form(c)
    if not staged_decode:
        if (logn in (10, 11, 12) and g == 5 and logm == logn - 2 and cp == n // 4 and 1 <= s <= RX_SMAX
                and 2 <= d <= RX_DPT * t and 1 <= p <= t and _wide_shm(c) <= LDS_LIMIT):
            return ("fused-wide", logn)
        if logn == 9 and (logm, g) == (7, 5) and cp == 128 and s <= RX_SMAX and d <= 256 and p <= 64:
            return ("fused-narrow",)
    return ("staged", logn, (logm, g), "rx_stream2" if logn == 9 else "rx_kernel")


# ------------------------------------------------------------------ streams
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def as_i16(x):
    """complex128 -> interleaved int16 of x * I16_SCALE, rounded (test_gpu_stream.to_i16 of x * 200)."""
    r = np.empty(2 * len(x), np.int16)
    r[0::2] = np.clip(np.round(x.real * I16_SCALE), -32768, 32767)
    r[1::2] = np.clip(np.round(x.imag * I16_SCALE), -32768, 32767)
    return r


def as_f64(x16):
    return x16[0::2].astype(np.float64) + 1j * x16[1::2].astype(np.float64)


def cfo_bound(c):
    """The streams' CFO bound: 0.004 turns a 449-sample template 1.8 times and
    the oracle's own walk finds a third of the frames; 0.15 / L keeps the
    template within 0.15 turns."""
    return min(0.004, 0.15 / c["pr_sin_len"])


def _impaired(c, nf, seed):
    x = impaired_stream(c, nf, seed, gap_max=4096, snr_db=25.0, cfo_max=cfo_bound(c))[0]
    x = np.ascontiguousarray(x, np.complex128)
    x16 = as_i16(x)
    return _frozen(x, x16, as_f64(x16))


@functools.lru_cache(maxsize=None)
def walker_streams(name):
    """One walker case: dict(cfg, x (the impaired stream), x16 (its int16
    form), xd (x16's samples as complex128))."""
    c = walker_config(*WALKER[name])
    x, x16, xd = _impaired(c, WALKER_FRAMES, WALKER_SEED)
    return dict(cfg=c, x=x, x16=x16, xd=xd)


@functools.lru_cache(maxsize=None)
def capture(size):
    """The wire capture of one T2 size (the frames do not depend on
    pr_sin_len): (complex128 samples, interleaved int16)."""
    c = walker_config(size, 128)
    return _frozen(*capture_stream(c, CAPTURE_FRAMES, WALKER_SEED + size))


@functools.lru_cache(maxsize=None)
def decode_streams(name):
    c = DECODE[name]
    x, x16, xd = _impaired(c, DECODE_FRAMES, DECODE_SEED)
    return dict(cfg=c, x=x, x16=x16, xd=xd)


def small_ring(c):
    return 2 * O.geometry(c)["frame_len"]


def chunks(c):
    """The chunk sizes of a walker case: automatic, about 1.3 frames, 5 frames."""
    flen = O.geometry(c)["frame_len"]
    return 0, flen * 13 // 10 + 7, 5 * flen


def walk(c, x, ring=None):
    """The oracle's walk and the ring ends it passed before its last frame
    (each refill moves the ring end on by R at the most: a frame at or past
    k R lies behind at least k of them)."""
    pbs = O.stream_walk_ring(c, x, ring=ring)[0]
    r = O.ring_len(c) if ring is None else ring
    return pbs, (int(pbs[-1]) // r if r and len(pbs) else 0)


def frame_at(x, pb, span):
    out = np.zeros(span, np.complex128)
    lo, hi = max(pb, 0), min(pb + span, len(x))
    if hi > lo:
        out[lo - pb:hi - pb] = x[lo:hi]
    return out


def edge_distance(c, x, pbs):
    """The least distance of any oracle point of the frames at pbs from its nearest decision edge."""
    g = O.geometry(c)
    span = g["preamble_len"] + g["message_len"]
    best = np.inf
    for pb in pbs:
        cons = O.decode_frame(c, frame_at(x, int(pb), span))[1]
        best = min(best, float(distance_to_threshold(c["mod_type"], cons).min()))
    return best


# ------------------------------------------------------------------ the last lag of the preamble search
EDGE_SEED = 77
EDGES = ("in", "out")


def edge_range(c, where):
    """The lags (from the T2 hit) the first passing lag of an edge stream must
    fall in. "in": the search's last lags (FFT search: its last window, which
    is a partial one on most cases; direct: the last 8). "out": just past lag
    C - 1, where nothing may be found (FFT search: the lags a last window
    taken whole would hold; direct: the next 32). None where "out" has no
    such lag (the last window is a whole one)."""
    cyc = 2 * c["t2sin_size"] + c["pr_sin_len"]
    if expected_walker(c)[4] == "direct":
        return (cyc - 8, cyc - 1) if where == "in" else (cyc, cyc + 31)
    q, last = WALK_FFT_M + 1 - c["pr_sin_len"], windows(c)[-1]
    if where == "in":
        return cyc - last, cyc - 1
    return (cyc, cyc - last + q - 1) if last < q else None


def _first_pass(c, x, cycles):
    """The first lag from sample 0 whose ratio passes pr_level, by the serial FP64 recurrence, over `cycles` lags."""
    from detector_cases import find_corr_ref
    cor, _ = find_corr_ref(x, len(x), 0, O.preamble_setup(c)[2], cycles)
    hit = np.nonzero(cor > c["pr_level"] / 1000)[0]
    return int(hit[0]) if len(hit) else None


@functools.lru_cache(maxsize=None)
def edge_stream(name, where):
    """A T2 marker in block 0 of the continuous walk's grid, silence, then the
    frame's preamble and message placed so that the first lag whose ratio
    passes lies in edge_range: dict(cfg, x, lag, range), or None. "in": the
    frame is the search's last lags' to find; "out": the search ends before
    it, the walk moves on by a message, and the frame is not located."""
    from common import payload
    c = walker_config(*WALKER[name])
    rng = edge_range(c, where)
    if rng is None:
        return None
    g = O.geometry(c)
    size, cyc = c["t2sin_size"], 2 * c["t2sin_size"] + c["pr_sin_len"]
    fr = O.frame_write(c, payload(g["bytes_per_frame"], EDGE_SEED))
    marker, rest = fr[:size], fr[size:]
    target = (rng[0] + rng[1] + 1) // 2
    p = target
    for _ in range(40):  # the ratio passes a few samples before the preamble's first: move it until the lag is right
        x = np.zeros(p + len(rest) + g["frame_len"], np.complex128)
        x[:size] = marker
        x[p:p + len(rest)] = rest
        x = O.awgn(x, 10 ** (-25.0 / 20), seed=EDGE_SEED)
        lag = _first_pass(c, x, cyc + WALK_FFT_M)
        if lag is not None and rng[0] <= lag <= rng[1]:
            x.setflags(write=False)
            return dict(cfg=c, x=x, lag=lag, range=rng)
        p += target - lag if lag is not None else 1
    raise AssertionError(f"{name} {where}: no placement puts the first passing lag in {rng}")
