"""Fixtures of the batched rx's geometry tests (tests/test_gpu_rx_geometry.py:
ofdm_rx_demod, ofdm_rx_demod_i16, ofdm_rx_demod_read and ofdm_rx_demod_soft
on every non-stream rx kernel instance and on geometries off the D = N/2
diagonal, and one noise-free ofdm_tx_modulate with the int16 output per
geometry; tx's other instances and branches are tests/tx_cases.py's. The
fixtures themselves are checked on the CPU in tests/test_rx_geometry_cases.py).
No torch, no GPU: numpy and the oracle.

- CASES: the geometry table, overrides of O.DEFAULT. Per FFT size one case
  that fits the register window (S <= 8) and one that is staged (S > 8); the
  rest aim at a lane mask, a packing branch or a few-frame kernel.
- expected_instance: rx_dispatch / rx_soft_dispatch (csrc/ofdm_kernels.hip)
  restated: which kernel instance a launch takes. body_branches: the uniform
  predicates of csrc/ofdm_rx_body.inc a launch takes.
- runs: the (case, frame count, input, entry) launches of the GPU module.
- inputs / i16_input / channel: the samples, payloads and divisors of a case.
"""
import functools

import numpy as np

import oracle as O
from common import cfg as mkcfg, distance_to_threshold, payload

LDS_LIMIT = 160 * 1024
RX_SMAX, RX_DPT = 8, 4      # ofdm_internal.hpp: register window (symbols), data carriers per thread
FEW = 3                     # frames of the few-frame launches
SNR_DB, NOISE_SEED = 12.0, 3
STRIDE_EXTRA = 3            # frame_stride = message_len + 3: frames are not contiguous
EDGE_BAR = 1e-7             # every oracle point at least this far from its nearest decision edge
GAP_F64 = complex(np.nan, np.nan)  # what the samples between frames hold: never read as data
GAP_I16 = -32768


def _case(N, D, P, cp, k, S, aim):
    kw = dict(fft_size=N, num_data_subc=D, num_pilot_subc=P, cp_size=cp, mod_type=k, num_symb=S)
    if N + cp < O.DEFAULT["pr_sin_len"]:  # the context's preamble template must fit the preamble
        kw["pr_sin_len"] = 64
    return f"N{N}-D{D}-P{P}-cp{cp}-k{k}-S{S}", mkcfg(O.DEFAULT, **kw), aim


# (name, config, what it aims at)
_TABLE = [
    _case(64, 8, 2, 64, 1, 7, "D = T = 8, cp = N, 7 bytes per frame: byte-wise pack at k = 1"),
    _case(64, 24, 6, 7, 6, 3, "the last group of every thread masked at T = 8, odd cp, k = 6"),
    _case(64, 32, 8, 3, 6, 40, "staged: per-symbol pack at k = 6, channel from memory, P = T"),
    _case(128, 56, 14, 1, 4, 2, "cp = 1, a partial last group at T = 16, P near T"),
    _case(128, 64, 4, 16, 2, 17, "staged: channel from memory, decisions of the whole frame in LDS"),
    _case(256, 104, 4, 33, 8, 5, "k = 8, a partial last group at T = 32"),
    _case(256, 120, 30, 0, 4, 9, "staged, cp = 0, P near T, a partial last group"),
    _case(512, 72, 6, 5, 2, 7, "D % 64 != 0: the fast emit declines; 126 bytes per frame: byte-wise pack at k = 2"),
    _case(512, 40, 2, 512, 4, 8, "D < T: idle waves in the emit; cp = N; P = 2"),
    _case(512, 248, 62, 127, 1, 35, "staged: per-symbol pack at k = 1 (S*D > 16 N), 1085 bytes per frame"),
    _case(1024, 328, 8, 3, 6, 4, "rx_wide_kernel<10> on few frames; k = 6; D no multiple of T"),
    _case(1024, 504, 126, 255, 2, 9, "staged at LOGN 10, P near T"),
    _case(2048, 8, 2, 0, 2, 8, "D far below T; S*T > 1024: the persistent kernel on few frames too"),
    _case(2048, 1000, 50, 511, 4, 2, "rx_wide_kernel<11> on few frames"),
    _case(2048, 1000, 50, 511, 4, 10, "staged at LOGN 11"),
    _case(4096, 2040, 204, 1023, 2, 1, "rx_wide_kernel<12> on few frames; one symbol"),
    _case(4096, 96, 4, 17, 8, 9, "staged at LOGN 12, k = 8, D < T"),
]
CASES = {name: c for name, c, _ in _TABLE}
AIMS = {name: aim for name, _, aim in _TABLE}
NAMES = list(CASES)
# the cases whose FEW-frame f64 launches (with and without a channel) are meant for rx_wide_kernel
WIDE_CASES = ("N512-D72-P6-cp5-k2-S7", "N512-D40-P2-cp512-k4-S8", "N1024-D328-P8-cp3-k6-S4",
              "N2048-D1000-P50-cp511-k4-S2", "N4096-D2040-P204-cp1023-k2-S1")


def meant_instance(name, nf, i16, soft):
    """The instance a launch of the GPU module is in the table for: what
    expected_instance must answer on the device the test runs on."""
    c = CASES[name]
    logn, staged = c["fft_size"].bit_length() - 1, c["num_symb"] > RX_SMAX
    if soft:
        return "rx_soft_kernel", logn, staged, bool(i16)
    if name in WIDE_CASES and nf == FEW and not i16:
        return "rx_wide_kernel", logn, False, False
    return "rx_kernel", logn, staged, bool(i16)


# ------------------------------------------------------------------ the library's rules, restated
def layout_ok(N, D, P):
    """validate()'s walk over FFT_FORM's layout: every pilot and data bin inside [1, N), none twice."""
    used = set()

    def take(b):
        if b < 1 or b >= N or b in used:
            return False
        used.add(b)
        return True

    seg, step, half = D // P, D // P + 1, P // 2
    pos = 1 + seg
    for _ in range(half):
        if not take(pos) or not all(take(pos - seg + t) for t in range(seg)):
            return False
        pos += step
    pos = N - step * half
    for _ in range(half, P):
        if not take(pos) or not all(take(pos + 1 + t) for t in range(seg)):
            return False
        pos += step
    return True


def valid(c):
    """validate() (csrc/ofdm_create.cpp) and rx_dispatch's P <= T on one config."""
    N, D, P, k = c["fft_size"], c["num_data_subc"], c["num_pilot_subc"], c["mod_type"]
    S, cp = c["num_symb"], c["cp_size"]
    return (N in (64, 128, 256, 512, 1024, 2048, 4096) and P >= 2 and P % 2 == 0 and D % P == 0 and D % 8 == 0
            and (D * k) % 8 == 0 and D <= N // 2 and P <= min(N // 8, 256) and k in (1, 2, 4, 6, 8)
            and 0 <= cp <= N and S >= 1 and (D * c["num_pr_symb"]) % 8 == 0 and layout_ok(N, D, P)
            and 0 <= c["pr_sin_len"] <= (N + cp) * c["num_pr_symb"])


def rx_shm(c):
    """rx_kernel's / rx_soft_kernel's dynamic LDS (rx_shm: TwLds::SIZE = N/64 + 64, PADN = N)."""
    N, P, S = c["fft_size"], c["num_pilot_subc"], c["num_symb"]
    return 16 * (N + N + N // 64 + 64 + 2 * S * P) + 32 * 8


def rx_wide_shm(c):
    N, D, P, S = c["fft_size"], c["num_data_subc"], c["num_pilot_subc"], c["num_symb"]
    return 16 * (N // 64 + 64 + S * (N + N) + 2 * S * P) + 16 * 8 + S * D


def fits(c):
    return c["num_symb"] <= RX_SMAX and c["num_data_subc"] <= RX_DPT * (c["fft_size"] // 8)


def rx_wide_ok(c, nframes, num_cus):
    N, S = c["fft_size"], c["num_symb"]
    return N >= 512 and S >= 1 and S * (N // 8) <= 1024 and nframes <= num_cus // 2 and rx_wide_shm(c) <= LDS_LIMIT


def expected_instance(c, nframes, i16, soft, num_cus):
    """(family, LOGN, STAGED, I16) of one launch, as rx_dispatch and
    rx_soft_dispatch decide it; the few-frame kernel has no STAGED / I16 forms
    (both False). A geometry the library would refuse raises."""
    logn = c["fft_size"].bit_length() - 1
    if not valid(c) or c["num_data_subc"] > RX_DPT * (c["fft_size"] // 8) or nframes <= 0:
        raise ValueError("no launch")
    staged = not fits(c)
    if soft:
        family = "rx_soft_kernel"
    elif not i16 and not staged and rx_wide_ok(c, nframes, num_cus):
        return "rx_wide_kernel", logn, False, False
    else:
        family = "rx_kernel"
    if rx_shm(c) > LDS_LIMIT:
        raise ValueError("rx_shm over the LDS limit")
    return family, logn, staged, bool(i16)


def whole_frame_dec(c):
    return c["num_symb"] * c["num_data_subc"] <= 16 * c["fft_size"]


def chan_lds(c):
    """Whether a channel divisor goes to LDS behind the frame's decisions."""
    D = c["num_data_subc"]
    return ((c["num_symb"] * D + 15) & ~15) + 16 * D <= 16 * c["fft_size"]


BRANCHES = ("whole_frame_dec false", "chan_lds false with a channel", "bytes per frame % 4 != 0 at k in 1,2,4,8",
            "k = 6 in the per-symbol staged pack", "D < T", "D no multiple of T at T < 64")


def body_branches(c, instance, with_chan):
    """The conditions of BRANCHES that one launch of rx_kernel / rx_soft_kernel
    meets (the few-frame kernel has its own body: none)."""
    family, _, staged, _ = instance
    if family == "rx_wide_kernel":
        return set()
    D, k, T = c["num_data_subc"], c["mod_type"], c["fft_size"] // 8
    bpf = O.geometry(c)["bytes_per_frame"]
    got = set()
    if staged and not whole_frame_dec(c):
        got.add(BRANCHES[0])
        if k == 6:
            got.add(BRANCHES[3])
    if with_chan and not chan_lds(c):
        assert staged  # S <= 8 and D <= N/2 leave room for the channel
        got.add(BRANCHES[1])
    if not staged and k in (1, 2, 4, 8) and bpf % 4:
        got.add(BRANCHES[2])
    if D < T:
        got.add(BRANCHES[4])
    if T < 64 and D % T:
        got.add(BRANCHES[5])
    return got


def frame_counts(c, num_cus):
    """FEW frames; from N = 512 on also more than rx_wide_ok takes: the persistent kernel."""
    return (FEW,) if c["fft_size"] < 512 else (FEW, num_cus // 2 + 2)


def runs(name, num_cus):
    """The rx launches of one case in the GPU module:
    [(entry, frames, i16, soft, with_chan)]."""
    c = CASES[name]
    out = []
    for nf in frame_counts(c, num_cus):
        out += [("rx", nf, False, False, False), ("rx_read", nf, False, False, True)]
    out += [("rx_i16", FEW, True, False, False), ("rx_soft", FEW, False, True, False),
            ("rx_soft", FEW, True, True, False)]
    return out


# ------------------------------------------------------------------ inputs
# Cases whose first payload left an oracle point of the persistent launch's
# ~1e5 points (64-QAM, 256-QAM) closer than EDGE_BAR to a decision edge: the
# next payload seed that does not (tests/test_rx_geometry_cases.py checks it).
SEED_BUMP = {"N1024-D328-P8-cp3-k6-S4": 1, "N4096-D96-P4-cp17-k8-S9": 1}


def case_seed(name):
    return 40 + NAMES.index(name) + 100 * SEED_BUMP.get(name, 0)


def stride_of(c):
    return O.geometry(c)["message_len"] + STRIDE_EXTRA


@functools.lru_cache(maxsize=2)
def inputs(name, nf):
    """nf frames of one case: O.tx_batch at stride_of(c), O.awgn at Es/N0 =
    SNR_DB over it, NaN between the frames. dict(cfg, nf, stride, data, ref (not
    the payload: many bit errors to count), clean, iq, cons / bytes (the
    oracle's rx of iq), edge (the least distance of a point of `cons` from a
    decision edge)). The first frames do not depend on nf."""
    c = CASES[name]
    g = O.geometry(c)
    stride, msg, bpf = stride_of(c), g["message_len"], g["bytes_per_frame"]
    seed = case_seed(name)
    data = np.concatenate([payload(bpf, seed * 1000 + f) for f in range(nf)])
    ref = np.concatenate([payload(bpf, seed * 1000 + 500 + f) for f in range(nf)])
    clean = np.zeros(nf * stride, np.complex128)
    clean[:(nf - 1) * stride + msg] = O.tx_batch(c, data, nf, stride, threads=8)
    es = float(np.mean(np.abs(O.constellation(c["mod_type"])) ** 2))
    iq = O.awgn(clean, np.sqrt(es / 10 ** (SNR_DB / 10)), seed=NOISE_SEED, threads=8)
    iq.reshape(nf, stride)[:, msg:] = GAP_F64
    cons, obytes, _ = O.rx_batch(c, iq, nf, stride, threads=8)
    edge = float(distance_to_threshold(c["mod_type"], cons).min())
    for a in (data, ref, clean, iq, cons, obytes):
        a.setflags(write=False)
    return dict(cfg=c, nf=nf, stride=stride, data=data, ref=ref, clean=clean, iq=iq, cons=cons, bytes=obytes,
                edge=edge)


def bit_errors(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


# (I, Q) of the extreme samples written into frame 1 of the int16 input
EXTREMES = ((32767, -32768), (-32768, 32767), (-32768, -32768), (32767, 32767))


def extreme_positions(c):
    """Sample offsets in a frame of the extreme int16 values: the first and a
    middle sample of symbol 0's body, a sample of the last symbol, the frame's
    last sample."""
    N, cp, S = c["fft_size"], c["cp_size"], c["num_symb"]
    L = N + cp
    return (cp, cp + N // 2 + 1, (S - 1) * L + cp + 5, S * L - 1)


@functools.lru_cache(maxsize=2)
def i16_input(name):
    """The FEW-frame input in the wire format (FRAME_FORM::get_int16: x mult,
    truncated), the most negative value between the frames, +-32767 / -32768 in
    four samples of frame 1. dict(x16 (interleaved int16), iq (those integers
    as complex128), cons / bytes (the oracle's rx of iq), edge, peak (the
    largest |int16| outside the gaps and the extremes))."""
    base = inputs(name, FEW)
    c, stride = base["cfg"], base["stride"]
    msg = O.geometry(c)["message_len"]
    noisy = np.where(np.isnan(base["iq"]), 0.0, base["iq"])
    x16 = O.get_int16(noisy, c["mult"]).reshape(FEW, stride, 2)
    peak = int(np.abs(x16[:, :msg].astype(np.int32)).max())
    x16[:, msg:] = GAP_I16
    for pos, v in zip(extreme_positions(c), EXTREMES):
        x16[1, pos] = v
    x16 = np.ascontiguousarray(x16.reshape(-1))
    w = x16.astype(np.float64)
    iq = w[0::2] + 1j * w[1::2]
    cons, obytes, _ = O.rx_batch(c, iq, FEW, stride)
    edge = float(distance_to_threshold(c["mod_type"], cons).min())
    for a in (x16, iq, cons, obytes):
        a.setflags(write=False)
    return dict(x16=x16, iq=iq, cons=cons, bytes=obytes, edge=edge, peak=peak)


def channel(name, nf):
    """A divisor per frame and carrier (chan_stride = D), as
    test_rx_demod_read_one_launch_equals_rx_with_and_without_channel builds it;
    the first frames do not depend on nf."""
    D = CASES[name]["num_data_subc"]
    phase = np.random.default_rng(case_seed(name) + 7000).uniform(-0.3, 0.3, nf * D)
    ampl = np.random.default_rng(case_seed(name) + 8000).uniform(0.8, 1.2, nf * D)
    return np.exp(1j * phase) * ampl
