"""Frequency-selective channels on the GPU: ofdm_chan_estimate_ls and
ofdm_soft_demap_csi against the numpy model of tests/csi_model.py, the coded
link through a spectral notch end to end, one case behind the sync chain,
graph capture of the receive chain, and the error returns.

Bars. The LS estimate against the model: 1e-9 * max|H_model| per frame, the
project's parity bar for IQ values (the kernel applies 1/phys after the sum
over the preamble symbols: a reordering of roundings); csi = |H|^2 within
2e-9 * max|H|^2, its first-order image. The demapper on identical inputs:
soft_model's check_f32 / check_i8 with the absolute bar s * 1e-13 per element,
s = scale * frame_scale * csi (the product of three doubles adds less than
4e-15 * s at |x| <= 3 to the flat kernel's 1e-14). Erasures are bit-exact."""
import functools

import numpy as np
import pytest

import csi_model as CM
import fec_model as F
import interleave_model as IM
import oracle as O
import soft_model as SM
from common import B, CC, CHANNEL_CASES, D, EXTRA, TAPS_ECHO, TAPS_NOTCH, cfg, channel_frames
from test_gpu_graph import replay_protocol
from test_gpu_soft import flat_points

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

PAD = 64
SENT = 9.0       # test_gpu_graph's sentinels (replay_protocol refills with them)
SENT_INT = 77
TAPS = {"echo": TAPS_ECHO, "notch": TAPS_NOTCH}
FMTS = {"f32": (M.LLR_F32, torch.float32), "i8": (M.LLR_I8, torch.int8)}

_m = {}


def modem(p):
    key = repr(sorted(p.items()))
    if key not in _m:
        _m[key] = M.Modem(p, 0)
    return _m[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def sentinel(n, dtype):
    if dtype == torch.complex128:
        return torch.full((n,), complex(SENT, SENT), dtype=dtype, device="cuda")
    return torch.full((n,), SENT if dtype.is_floating_point else SENT_INT, dtype=dtype, device="cuda")


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ------------------------------------------------------------------ 1. the LS estimate
LS_CASES = {"N64_k1": (EXTRA["N64_k1"], 3, (0, 1, 3, 64)), "N128_k4_s3": (EXTRA["N128_k4_s3"], 3, (0, 1, 3)),
            "D": (D, 3, (0, 1, 3)), "D_pr2": (cfg(D, num_pr_symb=2), 3, (0, 1, 3)),
            "D384": (cfg(D, num_data_subc=384), 3, (0, 1, 3)), "B": (B, 2, (0, 1, 3)), "C": (CC, 1, (0, 1, 3))}


@pytest.mark.parametrize("taps", list(TAPS))
@pytest.mark.parametrize("name", list(LS_CASES))
def test_ls_estimate_equals_the_model(name, taps):
    p, nf, smooths = LS_CASES[name]
    m = modem(p)
    Dn = p["num_data_subc"]
    regions, _ = channel_frames(p, nf, 71, TAPS[taps], offset=0, snr_db=34.0, cfo_max=0.0)
    n = regions.shape[1]
    stride, cs, ws = n + 7, Dn + 5, Dn + 3
    hx = np.zeros((nf, stride), np.complex128)
    hx[:, :n] = regions
    x = dev(hx.reshape(-1))
    for w in smooths:
        chan = sentinel(nf * cs + PAD, torch.complex128)
        csi = sentinel(nf * ws + PAD, torch.float64)
        m.chan_estimate_ls(x, nf, stride, chan, csi, smooth=w, chan_stride=cs, csi_stride=ws)
        hchan, hcsi = host(chan), host(csi)
        assert np.all(hchan[nf * cs:] == complex(SENT, SENT)) and np.all(hcsi[nf * ws:] == SENT), "wrote past the end"
        gc, gw = hchan[:nf * cs].reshape(nf, cs), hcsi[:nf * ws].reshape(nf, ws)
        assert np.all(gc[:, Dn:] == complex(SENT, SENT)) and np.all(gw[:, Dn:] == SENT), "wrote into a stride gap"
        for f in range(nf):
            H, c = CM.ls_estimate(p, regions[f], w)
            top = float(np.abs(H).max())
            eh = float(np.abs(gc[f, :Dn] - H).max())
            ec = float(np.abs(gw[f, :Dn] - c).max())
            print(f"{name} {taps} w={w} frame {f}: |H err| {eh / top:.2e} of max|H|, csi err {ec / top ** 2:.2e}")
            assert eh <= 1e-9 * top
            assert ec <= 2e-9 * top ** 2
        if w == smooths[-1]:  # each output alone writes exactly itself
            only_c, only_w = sentinel(nf * cs + PAD, torch.complex128), sentinel(nf * ws + PAD, torch.float64)
            m.chan_estimate_ls(x, nf, stride, only_c, None, smooth=w, chan_stride=cs, csi_stride=ws)
            m.chan_estimate_ls(x, nf, stride, None, only_w, smooth=w, chan_stride=cs, csi_stride=ws)
            assert same_bits(host(only_c), hchan) and same_bits(host(only_w), hcsi)
    assert same_bits(host(x), hx.reshape(-1)), "the input was modified"


# ------------------------------------------------------------------ 2. the weighted demapper
def csi_points(k, nf, npts):
    """flat_points (random in [-3,3]^2 plus the designed ties) with the first
    three points of frame 0 made non-finite."""
    pts, designed = flat_points(k, nf * npts)
    pts = pts.copy().reshape(nf, npts)
    pts[0, 0], pts[0, 1], pts[0, 2] = complex(np.nan, 0.25), complex(0.25, -np.inf), complex(np.inf, np.nan)
    return pts, designed.reshape(nf, npts)


def csi_weights(nf, Dn, seed):
    """Uniform in [0.01, 4]; carriers 3..6 of frame 0 (the shared vector) hold
    0, a negative value, inf and NaN, carrier 7 of the last frame -0.0."""
    w = np.random.default_rng(seed).uniform(0.01, 4.0, (nf, Dn))
    w[0, 3:7] = (0.0, -1.5, np.inf, np.nan)
    w[nf - 1, 7] = -0.0
    return w


@pytest.mark.parametrize("geo", ["D-3", "N64-1", "N64-3"])
@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("k", SM.KS)
def test_soft_demap_csi_equals_the_model(k, fmt, geo):
    base, nf = {"D-3": (D, 3), "N64-1": (EXTRA["N64_k1"], 1), "N64-3": (EXTRA["N64_k1"], 3)}[geo]
    p = cfg(base, mod_type=k)
    m = modem(p)
    Dn, S = p["num_data_subc"], p["num_symb"]
    npts = Dn * S
    pts, designed = csi_points(k, nf, npts)
    w = csi_weights(nf, Dn, 10 * k + nf)
    fs = np.random.default_rng(3).uniform(0.25, 4.0, nf)
    d_pts, d_w, d_fs = dev(pts.reshape(-1)), dev(w.reshape(-1)), dev(fs)
    scale = 8.0
    for shared in (True, False):
        for with_fs in (False, True):
            wm = w[0] if shared else w
            sf = scale * (fs if with_fs else np.ones(nf))[:, None]
            L_ref = CM.csi_llr(k, pts, wm, sf)
            wfull = np.broadcast_to(np.tile(wm, S), pts.shape)
            erased = ~(np.isfinite(pts.real) & np.isfinite(pts.imag) & np.isfinite(wfull) & (wfull > 0))
            assert erased[0, :7].all() and (shared or erased[nf - 1, 7])
            bar = (sf * np.where(erased, 0.0, wfull) * 1e-13)[..., None] * np.ones(k)
            out = sentinel(nf * npts * k + PAD, FMTS[fmt][1])
            m.soft_demap_csi(d_pts, nf, d_w, out, scale, FMTS[fmt][0], frame_scale=d_fs if with_fs else None,
                             csi_stride=0 if shared else Dn)
            h = host(out)
            assert np.all(h[nf * npts * k:] == (SENT if fmt == "f32" else SENT_INT)), "wrote past the end"
            got = h[:nf * npts * k].reshape(nf, npts, k)
            what = f"csi k={k} {geo} shared={shared} frame_scale={with_fs}"
            if fmt == "f32":
                assert np.all(got[erased].view(np.uint32) == 0), "an erasure is not +0.0"
                SM.check_f32(got, L_ref, bar, what)
            else:
                assert np.all(got[erased] == 0)
                SM.check_i8(got, L_ref, bar, designed=np.repeat(designed[..., None], k, axis=-1), what=what)
    assert same_bits(host(d_pts), pts.reshape(-1)) and same_bits(host(d_w), w.reshape(-1)), "an input was modified"


@pytest.mark.parametrize("k,fmt,carriers,symbols,frames_per_cu", [(4, "f32", 256, 8, 8), (4, "i8", 256, 12, 6),
                                                                  (2, "i8", 384, 8, 8)])
def test_soft_demap_csi_several_tiles_per_workgroup(k, fmt, carriers, symbols, frames_per_cu):
    """With as many frames as resident workgroups (8 per CU) a workgroup walks
    all tiles of its frames: 8 symbols of D = 256 are two tiles, and 8*CUs + 5
    frames also take the grid-stride loop. With 6 frames per CU and 12 symbols
    (three tiles) a frame is split into a run of two tiles and a run of one.
    D = 256 divides the tile, so a lane keeps its weights from tile to tile;
    D = 384 (three tiles) reloads them."""
    p = cfg(D, mod_type=k, num_symb=symbols, num_data_subc=carriers)
    m = modem(p)
    nf = frames_per_cu * torch.cuda.get_device_properties(0).multi_processor_count + (5 if frames_per_cu == 8 else 0)
    Dn, npts = p["num_data_subc"], p["num_data_subc"] * symbols
    rng = np.random.default_rng(k)
    pts = rng.uniform(-3, 3, (nf, npts)) + 1j * rng.uniform(-3, 3, (nf, npts))
    w = csi_weights(nf, Dn, 77)
    fs = rng.uniform(0.25, 4.0, nf)
    wfull = np.tile(w, symbols)
    usable = np.isfinite(wfull) & (wfull > 0)
    L_ref = CM.csi_llr(k, pts, w, 8.0 * fs[:, None])
    bar = (8.0 * fs[:, None] * np.where(usable, wfull, 0.0) * 1e-13)[..., None] * np.ones(k)
    out = sentinel(nf * npts * k + PAD, FMTS[fmt][1])
    m.soft_demap_csi(dev(pts.reshape(-1)), nf, dev(w.reshape(-1)), out, 8.0, FMTS[fmt][0], frame_scale=dev(fs))
    h = host(out)
    assert np.all(h[nf * npts * k:] == (SENT if fmt == "f32" else SENT_INT)), "wrote past the end"
    got = h[:nf * npts * k].reshape(nf, npts, k)
    assert np.all(got[~usable] == 0)
    if fmt == "f32":
        SM.check_f32(got, L_ref, bar, f"csi {nf} frames")
    else:
        SM.check_i8(got, L_ref, bar, what=f"csi {nf} frames")


def test_soft_demap_csi_element_aligned_output():
    """An output that is only element aligned takes the element-wise stores."""
    k, nf = 6, 3
    p = cfg(D, mod_type=k)
    m = modem(p)
    Dn, npts = p["num_data_subc"], p["num_data_subc"] * p["num_symb"]
    pts, _ = csi_points(k, nf, npts)
    w = csi_weights(nf, Dn, 5)
    L_ref = CM.csi_llr(k, pts, w, 2.0)
    wfull = np.tile(w, p["num_symb"])
    bar = (2.0 * np.where(np.isfinite(wfull) & (wfull > 0), wfull, 0.0) * 1e-13)[..., None] * np.ones(k)
    d_pts, d_w = dev(pts.reshape(-1)), dev(w.reshape(-1))
    for fmt, off in (("f32", 1), ("i8", 3)):
        buf = sentinel(off + nf * npts * k + PAD, FMTS[fmt][1])
        m.soft_demap_csi(d_pts, nf, d_w, buf[off:], 2.0, FMTS[fmt][0])
        h = host(buf)
        sent = SENT if fmt == "f32" else SENT_INT
        assert np.all(h[:off] == sent) and np.all(h[off + nf * npts * k:] == sent)
        got = h[off:off + nf * npts * k].reshape(nf, npts, k)
        if fmt == "f32":
            SM.check_f32(got, L_ref, bar, "csi unaligned")
        else:
            SM.check_i8(got, L_ref, bar, max_excluded=1.0, what="csi unaligned")


# ------------------------------------------------------------------ 3. the link end to end
class SelectiveLink:
    """The receive chain of INTEGRATION.md "Frequency-selective channels" on
    csi_model.link_case frames (no CFO, offset 0: nothing for ofdm_sync_frames
    to do): chan_estimate_ls -> rx(chan = H, constell_out) -> soft_demap_csi
    (int8, scale 8) -> interleave_llr -> fec_decode -> scramble. weighted =
    False is the control leg: the same chain through ofdm_soft_demap. The tx
    of link_case has no scrambler, so the chain's last stage returns
    info ^ sequence(127)."""

    def __init__(self, p, rate, nf, weighted=True):
        self.p, self.m, self.rate, self.nf, self.weighted = p, modem(p), rate, nf, weighted
        g = O.geometry(p)
        self.Dn, self.S, self.k = p["num_data_subc"], p["num_symb"], p["mod_type"]
        self.npre, self.n = g["preamble_len"], g["preamble_len"] + g["message_len"]
        self.npts, self.cap = g["npts"], g["bytes_per_frame"] * 8
        self.nb = M.fec_max_info_bits(self.cap, rate)
        self.nbytes = (self.nb + 7) // 8
        c128, u8 = torch.complex128, torch.uint8
        self.x = torch.zeros((nf * self.n,), dtype=c128, device="cuda")
        self.H = sentinel(nf * self.Dn + PAD, c128)
        self.csi = sentinel(nf * self.Dn + PAD, torch.float64)
        self.cons = torch.zeros((nf * self.npts,), dtype=c128, device="cuda")
        self.llr = torch.zeros((nf * self.cap,), dtype=torch.int8, device="cuda")
        self.dellr = sentinel(nf * self.cap + PAD, torch.int8)
        self.dec = torch.zeros((nf * self.nbytes,), dtype=u8, device="cuda")
        self.out = sentinel(nf * self.nbytes + PAD, u8)
        wsz = M.fec_workspace_size(nf, self.nb)
        self.ws = torch.empty((wsz,), dtype=u8, device="cuda") if wsz else None

    def load(self, regions):
        self.x.copy_(torch.from_numpy(np.array(regions, copy=True).reshape(-1)))  # (the case's arrays are read-only)

    def run(self):
        m, nf = self.m, self.nf
        m.chan_estimate_ls(self.x, nf, self.n, self.H, self.csi)
        m.rx(self.x[self.npre:], nf, frame_stride=self.n, chan=self.H, chan_stride=self.Dn, constell_out=self.cons)
        if self.weighted:
            m.soft_demap_csi(self.cons, nf, self.csi, self.llr, 8.0, M.LLR_I8)
        else:
            m.soft_demap(self.cons, nf * self.npts, self.llr, 8.0, M.LLR_I8)
        m.interleave_llr(self.llr, nf * self.S, self.dellr, M.IL_INVERSE, fmt=M.LLR_I8)
        m.fec_decode(self.dellr, nf, self.nb, self.rate, self.dec, fmt=M.LLR_I8, llr_stride=self.cap,
                     workspace=self.ws)
        m.scramble(self.dec, nf, self.nb, self.out, seed=127)

    def lost(self, info):
        h = host(self.out)
        assert np.all(h[self.nf * self.nbytes:] == SENT_INT)
        want = F.pack(IM.scramble(info, 127))
        return int(np.any(h[:self.nf * self.nbytes].reshape(self.nf, self.nbytes) != want, axis=1).sum())


@functools.lru_cache(maxsize=None)
def model_losses(name, nf):
    case = CM.link_case({"N128_k4_s3": EXTRA["N128_k4_s3"], "D": D}[name], TAPS_NOTCH, F.R12, nf, 18.0)
    return CM.link_decode(case, "ls")[0], CM.link_decode(case, "csi")[0]


@pytest.mark.parametrize("name,nf", [("N128_k4_s3", 32), ("D", 6)])
def test_link_through_a_notch_end_to_end(name, nf):
    """Notch, rate 1/2, 18 dB: with the weight no codeword is lost; the same
    chain through ofdm_soft_demap loses at least half of what the CPU model of
    that leg loses (N128_k4_s3: 21 of 32, D: 6 of 6; the GPU chain lost the
    same counts)."""
    p = {"N128_k4_s3": EXTRA["N128_k4_s3"], "D": D}[name]
    case = CM.link_case(p, TAPS_NOTCH, F.R12, nf, 18.0)
    cpu_ls, cpu_csi = model_losses(name, nf)
    lost = {}
    for weighted in (True, False):
        link = SelectiveLink(p, F.R12, nf, weighted)
        assert link.nb == case["info_bits"]
        link.load(case["regions"])
        link.run()
        lost[weighted] = link.lost(case["info"])
    print(f"{name}: codewords lost of {nf}: CSI {lost[True]} (model {cpu_csi}), unweighted {lost[False]} (model {cpu_ls})")
    assert cpu_csi == 0 and lost[True] == 0
    assert lost[False] >= 1, "the control leg has no errors: the test no longer shows anything"
    assert 2 * lost[False] >= cpu_ls


# ------------------------------------------------------------------ 4. behind the sync chain
def test_ls_estimate_behind_the_sync_chain():
    """N1024_k4-echo-o17 (CFO, early cut, echo): sync_frames(SYNC_ALL), the LS
    estimate of the synced preamble, rx. No hard error in 49 152 bits; through
    the unit phasors of the same sync_frames call, thousands (the CPU oracle:
    0 against 24 425)."""
    name, p, taps, offset, seed, nf = next(c for c in CHANNEL_CASES if c[0] == "N1024_k4-echo-o17")
    m = modem(p)
    g = O.geometry(p)
    Dn, npre = p["num_data_subc"], g["preamble_len"]
    regions, data = channel_frames(p, nf, seed, taps, offset)
    n = regions.shape[1]
    x = dev(regions.reshape(-1))
    unit = torch.zeros((nf * Dn,), dtype=torch.complex128, device="cuda")
    H = torch.zeros_like(unit)
    m.sync_frames(x, nf, n, M.SYNC_ALL, chan_out=unit)
    m.chan_estimate_ls(x, nf, n, H)
    ref = dev(data)
    errs = {}
    for leg, chan in (("ls", H), ("unit", unit)):
        e = torch.zeros((1,), dtype=torch.int64, device="cuda")
        out = torch.zeros((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
        m.rx(x[npre:], nf, frame_stride=n, chan=chan, chan_stride=Dn, bytes_out=out, ref=ref, bit_errors=e)
        errs[leg] = int(np.unpackbits(host(out) ^ data).sum())
        assert errs[leg] == int(e.item())
    print(f"{name}: hard errors in {data.size * 8} bits: LS {errs['ls']}, unit phasors {errs['unit']}")
    assert data.size * 8 == 49152
    assert errs["ls"] == 0
    assert errs["unit"] >= 1000


# ------------------------------------------------------------------ 5. graph capture
def test_graph_capture_of_the_receive_chain():
    """test_gpu_graph.py's protocol on the chain of SelectiveLink (one stream,
    no parallel branches): replay 1 equals the eager run, replay 2 on
    overwritten inputs equals a fresh eager run; both decode to the payload."""
    p, nf = EXTRA["N128_k4_s3"], 16
    case = CM.link_case(p, TAPS_NOTCH, F.R12, 32, 18.0)
    link = SelectiveLink(p, F.R12, nf)
    n_out = nf * link.nbytes
    outs = {"out": link.out, "llr": link.dellr, "H": link.H, "csi": link.csi}
    live = {"out": n_out, "llr": nf * link.cap, "H": nf * link.Dn, "csi": nf * link.Dn}
    _, _, r1, r2, _ = replay_protocol(link.run, lambda c: link.load(case["regions"][c * nf:(c + 1) * nf]), outs, live)
    for c, r in ((0, r1), (1, r2)):
        want = F.pack(IM.scramble(case["info"][c * nf:(c + 1) * nf], 127))
        assert np.array_equal(r["out"][:n_out].reshape(nf, -1), want)


# ------------------------------------------------------------------ 6. errors
def test_invalid_arguments_launch_nothing():
    p = EXTRA["N128_k4_s3"]
    m = modem(p)
    L = M.lib()
    g = O.geometry(p)
    Dn, nf, n = p["num_data_subc"], 2, g["preamble_len"] + g["message_len"]
    npts, k = g["npts"], p["mod_type"]
    regions, _ = channel_frames(p, nf, 72, TAPS_ECHO, offset=0, cfo_max=0.0)
    x = dev(regions.reshape(-1))
    chan = sentinel(nf * Dn + PAD, torch.complex128)
    csi = sentinel(nf * Dn + PAD, torch.float64)
    pts = dev(flat_points(k, nf * npts)[0])
    w = dev(np.ones(nf * Dn))
    llr = sentinel(nf * npts * k + PAD, torch.float32)
    st = torch.cuda.current_stream().cuda_stream

    def ls(x_=x.data_ptr(), nf_=nf, smooth=0, c=chan.data_ptr(), cs=Dn, w_=csi.data_ptr(), ws=Dn):
        return L.ofdm_chan_estimate_ls(m.h, x_, nf_, n, smooth, c, cs, w_, ws, st)

    def soft(pts_=pts.data_ptr(), nf_=nf, w_=w.data_ptr(), ws=Dn, scale=1.0, fs=None, fmt=M.LLR_F32,
             out=llr.data_ptr()):
        return L.ofdm_soft_demap_csi(m.h, pts_, nf_, w_, ws, scale, fs, fmt, out, st)

    assert ls(x_=None) == -1
    assert ls(c=None, w_=None) == -1
    assert ls(smooth=-1) == -1 and ls(smooth=65) == -1
    assert ls(cs=Dn - 1) == -1 and ls(ws=Dn - 1) == -1
    assert ls(x_=x.data_ptr() + 8) == -1 and ls(c=chan.data_ptr() + 8) == -1 and ls(w_=csi.data_ptr() + 4) == -1
    assert ls(nf_=0) == 0
    assert soft(pts_=None) == -1 and soft(w_=None) == -1 and soft(out=None) == -1
    assert soft(fmt=2) == -1 and soft(fmt=-1) == -1
    for s in (0.0, -1.0, float("inf"), float("nan")):
        assert soft(scale=s) == -1
    assert soft(pts_=pts.data_ptr() + 8) == -1 and soft(out=llr.data_ptr() + 2) == -1
    assert soft(w_=w.data_ptr() + 4) == -1
    assert soft(ws=Dn - 1) == -1 and soft(ws=1) == -1
    assert soft(nf_=0) == 0
    torch.cuda.synchronize()
    for t in (chan, csi, llr):
        v = torch.view_as_real(t) if t.is_complex() else t
        assert bool((v == SENT).all()), "an invalid call launched something"
    # the same calls with valid arguments do write; an int8 output takes any address
    assert ls() == 0 and soft() == 0 and soft(ws=0) == 0
    assert soft(fmt=M.LLR_I8, out=llr.data_ptr() + 1) == 0
    torch.cuda.synchronize()
    assert not bool((torch.view_as_real(chan)[:nf * Dn] == SENT).all()) and not bool((llr[:nf * npts * k] == SENT).all())


def test_unsupported_geometries_launch_nothing():
    """k outside 1, 2, 4, 6, 8 (where ofdm_create lets such a context exist),
    and a preamble form whose pilots do not fit the LDS: OFDM_ERR_UNSUPPORTED
    before anything is launched."""
    import ctypes as C
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros((4096,), dtype=torch.complex128, device="cuda")
    out = sentinel(4096, torch.float32)
    for k in (3, 5, 7):
        h = C.c_void_p()
        prm = M.Params.make(**cfg(EXTRA["N64_k1"], mod_type=k))
        rc = M.lib().ofdm_create(C.byref(prm), 0, C.byref(h))
        if rc != 0:
            assert rc == -1
            continue
        assert M.lib().ofdm_soft_demap_csi(h, buf.data_ptr(), 1, buf.data_ptr(), 0, 1.0, None, M.LLR_F32,
                                           out.data_ptr(), st) == -2
        M.lib().ofdm_destroy(h)
    # config C with 64 preamble symbols: 4096 + 144 + 64*64 + 2048 = 10 384 complex values, 10 240 fit
    big = cfg(CC, num_pr_symb=64)
    h = C.c_void_p()
    prm = M.Params.make(**big)
    rc = M.lib().ofdm_create(C.byref(prm), 0, C.byref(h))
    assert rc == 0, "no context for 64 preamble symbols of config C: the LDS limit is not tested"
    n = (big["fft_size"] + big["cp_size"]) * big["num_pr_symb"]
    x = torch.zeros((n,), dtype=torch.complex128, device="cuda")
    csi = sentinel(big["num_data_subc"], torch.float64)
    assert M.lib().ofdm_chan_estimate_ls(h, x.data_ptr(), 1, n, 0, None, 0, csi.data_ptr(), big["num_data_subc"],
                                         st) == -2
    torch.cuda.synchronize()
    M.lib().ofdm_destroy(h)
    assert bool((csi == SENT).all()) and bool((out == SENT).all())
