"""Fixtures of tx's geometry tests (tests/test_gpu_tx_geometry.py:
ofdm_tx_modulate with and without the fused AWGN and the int16 output,
ofdm_fft_write and ofdm_tx_frames on every instance of tx_kernel the C ABI
reaches; the fixtures themselves are checked on the CPU in
tests/test_tx_cases.py). No torch, no GPU: numpy and the oracle.

- CASES: the geometry table, overrides of O.DEFAULT. tx takes what
  validate() (csrc/ofdm_create.cpp) takes: unlike rx it has no D <= N/2 and no
  P <= T limit.
- expected_instance: tx_launch_modes (csrc/ofdm_kernels.hip) restated. The C
  ABI reaches 35 instances of tx_kernel<LOGN, POINTS, NOISE, I16>: per LOGN
  6..12 <L,0,0,0>, <L,0,0,1>, <L,0,1,0>, <L,0,1,1> (ofdm_tx_modulate; the
  first two also ofdm_tx_frames, with the header set) and <L,1,0,0>
  (ofdm_fft_write). The other 21 (POINTS with NOISE or I16) are compiled, but
  no entry of include/ofdm_mi355x.h passes points together with a channel or
  an int16 output: they stay untested.
- branches: the uniform predicates of tx_kernel that one launch takes.
- runs: the launches of the GPU module.
- lowbias32 / awgn_hashes / awgn_noise: the AWGN definition (oracle/ofdm_oracle.c,
  orc_awgn_mt) restated; EDGE_COUNTERS: sample counters of AWGN_SEED whose
  Box-Muller inputs are extreme; edge_offset: the sample_offset that puts one
  on a given sample.
- inputs / noisy / points / fft_write_ref / frames_ref: payloads, points and
  the oracle's outputs of a case.
"""
import functools

import numpy as np

import oracle as O
from common import cfg as mkcfg, payload
from rx_geometry_cases import layout_ok

TX_MAX_GRID = 4096          # ofdm_internal.hpp: the workgroups of the largest tx grid
FEW, MANY = 3, 600          # frames: a few, and (at S = 7) more symbols than the grid holds
STRIDE_EXTRA = 3            # frame_stride = message_len + 3: frames are not contiguous
GAP_F64 = complex(9.0, 9.0)  # what the outputs hold between the frames: never written
GAP_I16 = 77
NOISE_STD, NOISE_SMALL, NOISE_LARGE = 0.3, 1e-6, 50.0  # the suite's level; (float)a.noise_scale at both ends
AWGN_SEED = (5 << 40) + 777
OFFSET0 = (3 << 32) + 1000003  # sample_offset of the launches that aim at no edge counter
INT16_BAND = 1e-9           # assert_int16_match's ambiguity band
INT16_BAND_SHARE = 1e-3     # at most this share of a launch's components may lie inside it


def _case(N, D, P, cp, k, S, aim, **more):
    kw = dict(fft_size=N, num_data_subc=D, num_pilot_subc=P, cp_size=cp, mod_type=k, num_symb=S, **more)
    if N + cp < O.DEFAULT["pr_sin_len"]:  # the context's preamble template must fit the preamble
        kw["pr_sin_len"] = 64
    return f"N{N}-D{D}-P{P}-cp{cp}-k{k}-S{S}", mkcfg(O.DEFAULT, **kw), aim


# (name, config, what it aims at)
# mult = 197 at N = 64 and 256: there sqrt(N) is an integer, and with the default 200 the samples n = 0, N/4, N/2,
# 3N/4 of every symbol (all twiddles +-1, +-i) times mult / sqrt(N) are integers whenever the constellation's
# coordinates are +-1 or a few thirds: up to 6 % of a launch inside assert_int16_match's band, whatever the payload.
# 256-QAM (fifteenths) with a mult coprime to 120 leaves those samples on an integer once in 120 times.
_TABLE = [
    _case(64, 32, 4, 5, 8, 7, "600 frames: 4200 symbols on 4096 workgroups, 4096 % 7 != 0; general cp; T = 8: no "
          "dead-group forms; the many-frame ofdm_tx_frames and ofdm_fft_write; the graph capture",
          t2sin_size=64, t2_sin_f1=5, t2_sin_f2=20, smooth=2, mult=197),
    _case(64, 32, 4, 5, 8, 200, "ofdm_tx_frames at LOGN 6 with the int16 output: frames long enough that the T2 "
          "symbol's exact zeros stay under the share of the band; a pilot amplitude that is no multiple of 1/30",
          t2sin_size=64, t2_sin_f1=5, t2_sin_f2=20, smooth=2, mult=197, pilot_ampl=2377),
    _case(64, 24, 6, 8, 8, 3, "cp = T (i_cp = 7); a word-aligned payload: also launched from an odd pointer",
          mult=197),
    _case(128, 120, 2, 1, 8, 2, "D > N/2 at k = 8: 120 of the payload stage's 128 bytes; cp = 1"),
    _case(128, 8, 2, 128, 6, 3, "cp = N (i_cp = 0); D < T; 6 bytes per symbol, 18 per frame: bytes for bps % 4 and "
          "bytes_per_frame % 4"),
    _case(256, 104, 4, 224, 6, 2, "cp = 7T (i_cp = 1); k = 6 with 78 bytes per symbol, 156 per frame: bytes for "
          "bps % 4 alone", mult=197),
    _case(256, 128, 8, 0, 8, 5, "cp = 0 (i_cp = 8)", mult=197),
    _case(512, 256, 8, 128, 4, 8, "the default config: DFT8_Z34, cp = N/4 (i_cp = 6); the three noise levels, the "
          "AWGN edge counters"),
    _case(512, 256, 8, 128, 4, 16, "ofdm_tx_frames at LOGN 9 with the int16 output: 16 symbols and mult = 197 (at "
          "200 the BPSK preamble's samples n = 0, N/4, N/2, 3N/4 are multiples of 12.5)", mult=197),
    _case(512, 40, 2, 511, 4, 2, "D < T: DFT8_Z2345; cp = N - 1: general cp over 8 trips of the CP loop"),
    _case(512, 448, 8, 3, 8, 2, "D > N/2 at k = 8 with T = 64: masks 0, the full first butterfly; general cp"),
    _case(1024, 512, 16, 256, 1, 3, "LOGN 10; BPSK"),
    _case(2048, 1024, 32, 512, 2, 3, "the benchmark's symbol (config B): both pruned forms in one workgroup; the "
          "three noise levels"),
    _case(4096, 2048, 64, 1023, 4, 1, "LOGN 12; general cp at T = 512; one symbol per frame: ofdm_tx_frames where "
          "only symbol 0 can write the header"),
]
CASES = {name: c for name, c, _ in _TABLE}
AIMS = {name: aim for name, _, aim in _TABLE}
NAMES = list(CASES)
GRID_CASE = "N64-D32-P4-cp5-k8-S7"        # the case launched on MANY frames
LEVEL_CASES = ("N512-D256-P8-cp128-k4-S8", "N2048-D1024-P32-cp512-k2-S3")
ODD_POINTER_CASE = "N64-D24-P6-cp8-k8-S3"
EDGE_CASE = "N512-D256-P8-cp128-k4-S8"    # cp in registers
FRAME_CASES = ("N64-D32-P4-cp5-k8-S200", "N512-D256-P8-cp128-k4-S16", "N4096-D2048-P64-cp1023-k4-S1")


# ------------------------------------------------------------------ the library's rules, restated
def valid(c):
    """validate() (csrc/ofdm_create.cpp) on one config: what ofdm_create, and so tx, takes."""
    N, D, P, k = c["fft_size"], c["num_data_subc"], c["num_pilot_subc"], c["mod_type"]
    S, cp, npr, t2 = c["num_symb"], c["cp_size"], c["num_pr_symb"], c["t2sin_size"]
    return (N in (64, 128, 256, 512, 1024, 2048, 4096) and P >= 1 and D >= P and D % P == 0 and P <= 256
            and k in (1, 2, 4, 6, 8) and 0 <= cp <= N and S >= 1 and npr >= 1 and (D * S * k) % 8 == 0
            and (D * k) % 8 == 0 and (D * npr) % 8 == 0 and layout_ok(N, D, P)
            and t2 >= 0 and (t2 == 0 or (0 <= c["t2_sin_f1"] < t2 and 0 <= c["t2_sin_f2"] < t2))
            and 0 <= c["pr_sin_len"] <= (N + cp) * npr)


ENTRIES = ("tx", "fft_write", "tx_frames")
INSTANCES = {("tx_kernel", logn, points, noise, i16) for logn in range(6, 13)
             for points, noise, i16 in ((False, False, False), (False, False, True), (False, True, False),
                                        (False, True, True), (True, False, False))}


def expected_instance(c, entry, noise, i16):
    """("tx_kernel", LOGN, POINTS, NOISE, I16) of one launch, as
    tx_launch_modes decides it from what the entry passes: ofdm_fft_write
    passes points and neither a channel nor an int16 output, ofdm_tx_frames
    passes no channel. A launch the C ABI cannot make raises."""
    if not valid(c) or entry not in ENTRIES:
        raise ValueError("no launch")
    if (entry == "fft_write" and (noise or i16)) or (entry == "tx_frames" and noise):
        raise ValueError(f"{entry} has no such argument")
    return "tx_kernel", c["fft_size"].bit_length() - 1, entry == "fft_write", bool(noise), bool(i16)


def dead_masks(c):
    """tx_dead_masks (ofdm_internal.hpp): per wave of the N/8 threads, bit i
    set when the 64 bins 64 w + lane + (N/8) i are all unused (bin 0 and the
    guard band); no waves' masks at T < 64."""
    N, D, P = c["fft_size"], c["num_data_subc"], c["num_pilot_subc"]
    T = N // 8
    pil, seg = O.layout(N, D, P)
    used = np.zeros(N, bool)
    used[pil] = True
    for s0 in seg:
        used[s0:s0 + D // P] = True
    return [sum(1 << i for i in range(8) if not used[64 * w + T * i:64 * w + T * i + 64].any())
            for w in range(T // 64)]


DFT8_Z2345, DFT8_Z34 = 0x3c, 0x18  # ofdm_fft.hpp
BRANCHES = {
    "by_word", "bytes: bps % 4", "bytes: bytes_per_frame % 4", "bytes: pointer",
    "cp_reg i_cp=0", "cp_reg i_cp=1", "cp_reg i_cp=6", "cp_reg i_cp=7", "cp_reg i_cp=8", "general cp",
    "DFT8_Z2345", "DFT8_Z34", "full", "no dead-group forms (T < 64)", "masks all 0",
    "nsym > TX_MAX_GRID", "nsym <= TX_MAX_GRID", "gridDim % S != 0", "header",
}


def branches(c, nframes, payload_alignment, entry="tx"):
    """The values of tx_kernel's uniform predicates in one launch, as strings
    of BRANCHES: by_word or each of its conditions that fails (bytes_per_frame
    = S bps, so that one never fails alone); cp in registers with its first CP
    register, or general cp; the first-butterfly form of each wave; the grid.
    ofdm_fft_write sets cp = 0 and reads no payload; ofdm_tx_frames sets the
    header."""
    N, D, k, S = c["fft_size"], c["num_data_subc"], c["mod_type"], c["num_symb"]
    T = N // 8
    cp = 0 if entry == "fft_write" else c["cp_size"]
    out = set()
    if entry != "fft_write":
        bps = D * k // 8
        fails = {what for what, bad in (("bytes: bps % 4", bps % 4), ("bytes: bytes_per_frame % 4", (bps * S) % 4),
                                        ("bytes: pointer", payload_alignment % 4)) if bad}
        out |= fails or {"by_word"}
    out.add(f"cp_reg i_cp={8 - cp // T}" if cp % T == 0 else "general cp")
    if T < 64:
        out.add("no dead-group forms (T < 64)")
    else:
        masks = dead_masks(c)
        for m in masks:
            out.add("DFT8_Z2345" if m & DFT8_Z2345 == DFT8_Z2345 else "DFT8_Z34" if m & DFT8_Z34 == DFT8_Z34
                    else "full")
        if not any(masks):
            out.add("masks all 0")
    nsym = nframes * S
    out.add("nsym > TX_MAX_GRID" if nsym > TX_MAX_GRID else "nsym <= TX_MAX_GRID")
    if min(nsym, TX_MAX_GRID) % S:
        out.add("gridDim % S != 0")
    if entry == "tx_frames":
        out.add("header")
    return out


# ------------------------------------------------------------------ the AWGN definition, restated
_M32 = np.uint64(0xFFFFFFFF)


def lowbias32(x):
    x = np.asarray(x, np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    return x ^ (x >> np.uint64(16))


def awgn_hashes(seed, g):
    """(h1, h2) of the sample counters g (orc_awgn_mt): h1 = H(lo(g) ^ H(hi(g) ^ k1) ^ k0),
    h2 = h1 * 0x9E3779B9 mod 2^32; u1 = ((h1 >> 8) + 1) 2^-24, u2 = (h2 >> 8) 2^-24."""
    g = np.asarray(g, np.uint64)
    k0 = lowbias32((seed & 0xFFFFFFFF) ^ 0x9E3779B9)
    k1 = lowbias32(((seed >> 32) + int(k0)) & 0xFFFFFFFF)
    h1 = lowbias32((g & _M32) ^ lowbias32((g >> np.uint64(32)) ^ k1) ^ k0)
    return h1, (h1 * np.uint64(0x9E3779B9)) & _M32


def awgn_noise(seed, g, noise_std):
    """The noise of samples g in double from the FP32 uniforms, as orc_awgn_mt has it."""
    h1, h2 = awgn_hashes(seed, g)
    u1 = ((h1 >> np.uint64(8)) + np.uint64(1)).astype(np.float32) * np.float32(2.0 ** -24)
    u2 = (h2 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * (noise_std * np.sqrt(0.5))
    th = 2.0 * np.pi * u2.astype(np.float64)
    return r * np.cos(th) + 1j * r * np.sin(th)


# kind: (hash, its top 24 bits). u1 = 2^-24: the largest radius, sqrt(2 ln 2^24) noise_std / sqrt(2);
# u1 = 1: radius 0; u2 = 0, 1/4, 1/2, 3/4: the quadrant boundaries of the GPU's sine and cosine.
EDGE_UNIFORMS = {"u1_min": ("h1", 0), "u1_one": ("h1", 0xFFFFFF), "u2_0": ("h2", 0), "u2_q1": ("h2", 1 << 22),
                 "u2_q2": ("h2", 1 << 23), "u2_q3": ("h2", 3 << 22)}
# The first counter of each kind below 2^27 for AWGN_SEED (edge_search; each has probability 2^-24 per sample)
EDGE_COUNTERS = {"u1_min": 12343645, "u1_one": 22360430, "u2_0": 15871555, "u2_q1": 7581222, "u2_q2": 6458858,
                 "u2_q3": 4117271}
MAX_RADIUS = float(np.sqrt(2.0 * np.log(2.0 ** 24)))  # in units of noise_std / sqrt(2)


def edge_search(seed=AWGN_SEED, limit=1 << 27, chunk=1 << 22):
    """The search EDGE_COUNTERS came from: {kind: first counter below limit} (a few seconds)."""
    found = {}
    for lo in range(0, limit, chunk):
        g = np.arange(lo, lo + chunk, dtype=np.uint64)
        h = dict(zip(("h1", "h2"), awgn_hashes(seed, g)))
        for kind, (which, top) in EDGE_UNIFORMS.items():
            if kind not in found:
                hit = np.flatnonzero((h[which] >> np.uint64(8)) == np.uint64(top))
                if hit.size:
                    found[kind] = int(g[hit[0]])
        if len(found) == len(EDGE_UNIFORMS):
            break
    return found


def edge_offset(c, kind, sym, j):
    """The sample_offset that puts EDGE_COUNTERS[kind] on sample j of symbol
    `sym` (counted over the launch: frame * S + symbol): g = sample_offset + sym L + j."""
    L = c["fft_size"] + c["cp_size"]
    assert 0 <= j < L
    off = EDGE_COUNTERS[kind] - sym * L - j
    assert off >= 0
    return off


def _edge_table():
    """(case, frames, kind, where, sym, j): every kind on the first CP sample
    and on the last body sample of a symbol of EDGE_CASE (cp in registers),
    each in a symbol of its own; the largest radius and radius 0 also past the
    first trip of the grid in GRID_CASE (symbol 4100: workgroup 4's second
    trip), on a CP sample of the general-cp path and on a last body sample."""
    c = CASES[EDGE_CASE]
    L, nsym = c["fft_size"] + c["cp_size"], FEW * c["num_symb"]
    out = []
    for i, kind in enumerate(EDGE_COUNTERS):
        out.append((EDGE_CASE, FEW, kind, "first CP sample", (3 * i + 1) % nsym, 0))
        out.append((EDGE_CASE, FEW, kind, "last body sample", (3 * i + 14) % nsym, L - 1))
    Lg = CASES[GRID_CASE]["fft_size"] + CASES[GRID_CASE]["cp_size"]
    out.append((GRID_CASE, MANY, "u1_min", "first CP sample", TX_MAX_GRID + 4, 0))
    out.append((GRID_CASE, MANY, "u1_one", "last body sample", TX_MAX_GRID + 4, Lg - 1))
    return out


EDGES = _edge_table()


def edge_at(name, offset):
    """The entries of EDGES that a launch of `name` at sample_offset `offset` places."""
    return [e for e in EDGES if e[0] == name and edge_offset(CASES[name], e[2], e[4], e[5]) == offset]


# ------------------------------------------------------------------ the launches
def frames_of(name):
    return MANY if name == GRID_CASE else FEW


def runs(name=None):
    """The launches of the GPU module:
    [(case, frames, entry, noise, i16, payload alignment, noise_std, sample_offset)].
    Every case: ofdm_tx_modulate in its four forms and ofdm_fft_write. On top:
    the other two noise levels (LEVEL_CASES), the four forms from an odd
    payload pointer (ODD_POINTER_CASE), both noisy forms at every entry of
    EDGES, ofdm_tx_frames without and with the int16 output on FEW frames
    (FRAME_CASES), and on MANY frames with it (GRID_CASE: its frames are too
    short for assert_int16_match, see int16_by_oracle)."""
    out = []
    for n in NAMES if name is None else [name]:
        nf = frames_of(n)
        forms = ((False, False, 0.0, 0), (False, True, 0.0, 0), (True, False, NOISE_STD, OFFSET0),
                 (True, True, NOISE_STD, OFFSET0))
        out += [(n, nf, "tx", noise, i16, 0, std, off) for noise, i16, std, off in forms]
        if n in LEVEL_CASES:
            out += [(n, nf, "tx", True, i16, 0, std, OFFSET0) for std in (NOISE_SMALL, NOISE_LARGE)
                    for i16 in (False, True)]
        if n == ODD_POINTER_CASE:
            out += [(n, nf, "tx", noise, i16, 1, std, off) for noise, i16, std, off in forms]
        for case, enf, kind, _, sym, j in EDGES:
            if case == n:
                assert enf == nf
                off = edge_offset(CASES[n], kind, sym, j)
                out += [(n, nf, "tx", True, i16, 0, NOISE_STD, off) for i16 in (False, True)]
        out.append((n, nf, "fft_write", False, False, 0, 0.0, 0))
        if n in FRAME_CASES:
            out += [(n, FEW, "tx_frames", False, i16, 0, 0.0, 0) for i16 in (False, True)]
        if n == GRID_CASE:
            out.append((n, MANY, "tx_frames", False, True, 0, 0.0, 0))
    return out


def int16_by_oracle(run):
    """Whether the int16 output of a noise-free launch is compared with the
    oracle's samples through assert_int16_match, and so has to leave its band
    all but empty. The T2 symbol has exact zeros (its imaginary part at n = 0
    and T2/2 at the least): 4 of the 1232 components of a GRID_CASE frame,
    three times the share allowed. That launch's int16 output is compared
    exactly instead: with trunc(mult x) of the launch's own f64 output."""
    name, nf, entry, noise, i16 = run[:5]
    return i16 and not noise and not (entry == "tx_frames" and nf == MANY)


# ------------------------------------------------------------------ inputs and the oracle's outputs
# Payload seeds: 70 + the case's index, raised by 100 per bump where the
# oracle's x mult left more than INT16_BAND_SHARE of a launch's components in
# assert_int16_match's band (tests/test_tx_cases.py checks it).
SEED_BUMP = {}


def case_seed(name):
    return 70 + NAMES.index(name) + 100 * SEED_BUMP.get(name, 0)


def stride_of(c):
    return O.geometry(c)["message_len"] + STRIDE_EXTRA


@functools.lru_cache(maxsize=4)
def inputs(name, nf):
    """nf frames of one case: dict(cfg, nf, stride, data, clean (the oracle's
    O.tx_batch, contiguous, as (nf, message_len)))."""
    c = CASES[name]
    g = O.geometry(c)
    data = payload(nf * g["bytes_per_frame"], case_seed(name))
    clean = O.tx_batch(c, data, nf, threads=8).reshape(nf, g["message_len"])
    for a in (data, clean):
        a.setflags(write=False)
    return dict(cfg=c, nf=nf, stride=stride_of(c), data=data, clean=clean)


@functools.lru_cache(maxsize=2)
def noisy(name, nf, noise_std, sample_offset):
    """O.awgn over the launch's nf S L contiguous samples (the kernel counts
    samples by sym * L + j whatever the frame stride), as (nf, message_len)."""
    clean = inputs(name, nf)["clean"]
    out = O.awgn(clean.reshape(-1), noise_std, seed=AWGN_SEED, sample_offset=sample_offset, threads=8)
    out = out.reshape(clean.shape)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=2)
def points(name, nf):
    """nf S D points that are no constellation points: seeded complex normal
    values, every 97th an exact zero and every 101st a negative zero."""
    c = CASES[name]
    n = nf * c["num_symb"] * c["num_data_subc"]
    rng = np.random.default_rng(case_seed(name) + 9000)
    pts = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    pts[5::97] = 0.0
    pts[7::101] = complex(-0.0, -0.0)
    pts.setflags(write=False)
    return pts


def fft_write_ref(c, pts, nf):
    """orc_fft_write frame by frame: (nf, S N)."""
    N, D, P, S = c["fft_size"], c["num_data_subc"], c["num_pilot_subc"], c["num_symb"]
    out = np.zeros((nf, N * S), np.complex128)
    for f in range(nf):
        O.lib().orc_fft_write(N, D, P, S, c["pilot_ampl"] / 1000, O._d(pts[f * D * S:(f + 1) * D * S].copy()),
                              O._d(out[f]))
    return out


@functools.lru_cache(maxsize=2)
def frames_ref(name, nf):
    """O.frame_write of each frame's payload: (nf, frame_len)."""
    c = CASES[name]
    bpf = O.geometry(c)["bytes_per_frame"]
    data = inputs(name, nf)["data"]
    out = np.stack([O.frame_write(c, data[f * bpf:(f + 1) * bpf]) for f in range(nf)])
    out.setflags(write=False)
    return out


def int16_band_share(x, mult):
    """The share of the components of x * mult inside assert_int16_match's band."""
    v = np.concatenate([x.real.ravel(), x.imag.ravel()]) * mult
    return float(np.mean(np.abs(v - np.round(v)) < INT16_BAND * np.maximum(1.0, np.abs(v))))
