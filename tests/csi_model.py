"""Numpy model of the frequency-selective channel path of
include/ofdm_mi355x.h ("frequency-selective channels"): the least-squares
per-carrier channel estimate of ofdm_chan_estimate_ls on top of the oracle's
FFT_FORM::read, and the channel-state weighted LLRs of ofdm_soft_demap_csi on
top of soft_model.ref_llr, with the erasure rule. Also the coded link over a
tapped channel that the CPU and the GPU tests share (link_case)."""
import functools

import numpy as np

import fec_model as F
import interleave_model as IM
import oracle as O
import soft_model as SM
from common import _apply_taps

SMOOTH_MAX = 64


def smooth_halves(raw, w):
    """Moving mean of half-width w that stays inside [0, D/2) or [D/2, D):
    raw[a..b] summed in ascending order, divided by the count."""
    D = len(raw)
    half = D // 2
    if w == 0:
        return raw.copy()
    H = np.empty(D, np.complex128)
    for c in range(D):
        lo, hi = (0, half) if c < half else (half, D)
        a, b = max(lo, c - w), min(hi - 1, c + w)
        acc = raw[a]
        for i in range(a + 1, b + 1):
            acc = acc + raw[i]
        H[c] = acc / (b - a + 1)
    return H


def ls_estimate(cfg, pre_region, smooth=0):
    """(H, csi) of one frame's preamble form: raw[c] = (1/npr) sum_s
    pr[s*D+c] / m[s*D+c] over FFT_FORM::read's points pr of the form and the
    preamble's own points m, smoothed; csi = re(H)^2 + im(H)^2."""
    assert 0 <= smooth <= SMOOTH_MAX
    D, npr = cfg["num_data_subc"], cfg["num_pr_symb"]
    assert D % cfg["num_pilot_subc"] == 0
    pre_len = O.geometry(cfg)["preamble_len"]
    pr = O.ofdm_fft(cfg, np.asarray(pre_region, np.complex128)[:pre_len], S=npr)
    m = O.preamble_setup(cfg)[1]
    raw = np.zeros(D, np.complex128)
    for s in range(npr):
        raw = raw + pr[s * D:(s + 1) * D] / m[s * D:(s + 1) * D]
    raw = raw / npr
    H = smooth_halves(raw, smooth)
    return H, H.real ** 2 + H.imag ** 2


def csi_llr(k, pts, csi, scale=1.0):
    """LLRs, shape pts.shape + (k,): ref_llr with s = scale * csi[i mod D]
    (csi: (D,) shared, or pts.shape[:-1] + (D,); scale broadcasts against
    pts). A point with a non-finite component, or a weight that is not finite
    and > 0, gives k exact +0.0."""
    pts = np.asarray(pts, np.complex128)
    csi = np.asarray(csi, np.float64)
    D, n = csi.shape[-1], pts.shape[-1]
    assert n % D == 0
    w = np.broadcast_to(np.tile(csi, n // D), pts.shape)
    ok = np.isfinite(pts.real) & np.isfinite(pts.imag) & np.isfinite(w) & (w > 0)
    s = np.broadcast_to(np.asarray(scale, np.float64), pts.shape) * np.where(ok, w, 0.0)
    L = SM.ref_llr(k, np.where(ok, pts, 0.0), s)
    L[~ok] = 0.0
    return L


def tap_response(cfg, taps):
    """The taps' DFT at the data bins, in the carrier order of the points."""
    N, D, P = cfg["fft_size"], cfg["num_data_subc"], cfg["num_pilot_subc"]
    seg = D // P
    _, sst = O.layout(N, D, P)
    bins = (sst[:, None] + np.arange(seg)[None, :]).reshape(-1)
    return sum(complex(g) * np.exp(-2j * np.pi * bins * d / N) for d, g in taps)


# ------------------------------------------------------------------ the coded link
@functools.lru_cache(maxsize=None)
def _link_case(cfg_items, taps, rate, nf, snr_db):
    cfg = dict(cfg_items)
    g = O.geometry(cfg)
    k, D, S = cfg["mod_type"], cfg["num_data_subc"], cfg["num_symb"]
    n, c, s = D * k, 16, max(k // 2, 1)
    cap = g["bytes_per_frame"] * 8
    nb = F.max_info_bits(cap, rate)
    info = np.random.default_rng(1).integers(0, 2, (nf, nb), dtype=np.uint8)
    frame = np.zeros((nf, cap), np.uint8)
    coded = F.encode(info, rate)
    frame[:, :coded.shape[1]] = coded
    sent = IM.interleave(frame, n, c, s)
    data = F.pack(sent)
    t2, rlen = cfg["t2sin_size"], g["preamble_len"] + g["message_len"]
    clean = np.zeros((nf, rlen), np.complex128)
    regions = np.zeros((nf, rlen), np.complex128)
    for f in range(nf):
        fr = _apply_taps(O.frame_write(cfg, data[f]), list(taps))
        clean[f] = fr[t2:t2 + rlen]
        if snr_db is None:
            regions[f] = clean[f]
        else:
            rms = float(np.sqrt(np.mean(np.abs(clean[f]) ** 2)))
            regions[f] = O.awgn(clean[f], rms * 10 ** (-snr_db / 20), seed=1000 + f)
    for a in (info, data, regions):
        a.setflags(write=False)
    return {"cfg": cfg, "rate": rate, "nf": nf, "info_bits": nb, "cap": cap, "block": (n, c, s), "info": info,
            "data": data, "regions": regions, "sent_points": O.mod(k, data.reshape(-1)).reshape(nf, D * S)}


def link_case(cfg, taps, rate, nf, snr_db=18.0):
    """nf frames, one codeword per frame (info bits from default_rng(1),
    encoded, zero-padded to the frame, interleaved with the default block),
    written by O.frame_write, convolved with `taps`; the [preamble | message]
    region starts at t2sin_size (no CFO, offset 0). AWGN `snr_db` below the
    tapped region's rms with seed 1000 + f (None: no noise). Cached and
    read-only. Keys: cfg, rate, nf, info_bits, cap, block, info (nf, nb) bits,
    data (nf, bytes_per_frame), regions (nf, n), sent_points (nf, D*S)."""
    return _link_case(tuple(sorted(cfg.items())), tuple(tuple(t) for t in taps), rate, nf, snr_db)


def link_decode(case, leg, scale=8.0):
    """The receive chain of `case` in numpy: the message's FFT_FORM::read
    points divided by the channel estimate, int8 LLRs at `scale`,
    deinterleave, Viterbi. leg: "unit" (chan_char_lq's unit phasors,
    unweighted LLRs), "ls" (the LS estimate, unweighted LLRs), "csi" (the LS
    estimate, LLRs weighted by |H|^2). Returns (codewords lost, hard bit
    errors of the equalised points against the sent ones, info bit errors)."""
    cfg, nf = case["cfg"], case["nf"]
    k, S = cfg["mod_type"], cfg["num_symb"]
    pre_len = O.geometry(cfg)["preamble_len"]
    n, c, s = case["block"]
    llr = np.zeros((nf, case["cap"]), np.int8)
    hard = 0
    for f in range(nf):
        reg = case["regions"][f]
        if leg == "unit":
            H, csi = O.chan_char_lq(cfg, reg[:pre_len]), None
        else:
            H, csi = ls_estimate(cfg, reg[:pre_len])
        E = O.ofdm_fft(cfg, reg[pre_len:], S=S) / np.tile(H, S)
        L = csi_llr(k, E, csi, scale) if leg == "csi" else SM.ref_llr(k, E, scale)
        llr[f] = SM.quant_i8(L).reshape(-1)
        got = np.unpackbits(O.demod(k, E)[0])[:case["cap"]]
        hard += int((got != np.unpackbits(case["data"][f])[:case["cap"]]).sum())
    bits, _ = F.viterbi(IM.deinterleave(llr, n, c, s), case["info_bits"], case["rate"])
    wrong = bits != case["info"]
    return int(np.any(wrong, axis=1).sum()), hard, int(wrong.sum())
