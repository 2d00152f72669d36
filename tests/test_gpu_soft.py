"""Soft-decision rx on the GPU: ofdm_soft_demap (flat points) and
ofdm_rx_demod_soft (LLRs fused into the batched rx) against the brute-force
numpy model of tests/soft_model.py.

Bars. Flat kernel, identical inputs: the FP64 evaluation of the (x-l)^2
differences at |x| <= 3 is good to 1e-14, so |L_gpu - L_ref| <= scale*1e-13
(10x) + one f32 rounding 2^-23*|L_ref|. Fused path against the oracle's
equalised points E: the model is 4-Lipschitz in the point (test_soft_model.py)
and the project's constellation parity bar is 1e-9 relative to max|E_f|, so
the absolute part is 4*s_f*1e-9*max|E_f|. int8: within 1 of the model
everywhere, equal wherever L_ref is farther than the absolute bar from a
rounding boundary (half-integers, +-127.5); at most 1e-4 of the values may be
that close, points built to sit on a tie not counted."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import soft_model as SM
from common import ALL_CONFIGS, D, cfg, payload
from test_gpu_decision_boundary import smith_div

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

FMTS = {"f32": (M.LLR_F32, np.float32, torch.float32), "i8": (M.LLR_I8, np.int8, torch.int8)}
PAD = 64          # sentinel elements past the output
SENTINEL = 77


def llr_buffer(n_elems, fmt):
    return torch.full((n_elems + PAD,), SENTINEL, dtype=FMTS[fmt][2], device="cuda")


def take_llr(buf, n_elems):
    """The launch's LLRs; the sentinel past them must have survived."""
    h = buf.cpu().numpy()
    assert np.all(h[n_elems:] == SENTINEL), "the kernel wrote past its output"
    return h[:n_elems]


# ------------------------------------------------------------------ 1. flat kernel
def special_axis_values(k):
    if k == 1:
        r = np.sqrt(0.5)
        return np.array([-r, r, 0.0, -0.0, 1.0, -1.0])
    lv = SM.levels(k)
    return np.concatenate([lv, (lv[1:] + lv[:-1]) / 2, [0.0, -0.0, 1.0, -1.0]])


@functools.lru_cache(maxsize=None)
def flat_points(k, n):
    """n points: random in [-3,3]^2, the last ones replaced by the designed
    set (every constellation point, every axis midpoint = tie, +-0, +-1; all of
    it at n = 4099, a random part of it below). Returns (points, designed mask)."""
    rng = np.random.default_rng(1000 * k + n)
    pts = rng.uniform(-3, 3, n) + 1j * rng.uniform(-3, 3, n)
    sp = special_axis_values(k)
    grid = (sp[None, :] + 1j * sp[:, None]).ravel()
    if k == 1:  # BPSK's tie is the line re + im = 0
        a = np.array([0.25, -1.5, 2.0, 0.7])
        grid = np.concatenate([grid, O.constellation(1), a - 1j * a])
    room = n if n < 4 else n // 2
    if len(grid) > room:
        grid = rng.choice(grid, room, replace=False)
    designed = np.zeros(n, bool)
    if len(grid):
        pts[n - len(grid):] = grid
        designed[n - len(grid):] = True
    return pts, designed


@pytest.mark.parametrize("scale", [1.0, 64.0])
@pytest.mark.parametrize("n", [1, 63, 4099])
@pytest.mark.parametrize("fmt", ["f32", "i8"])
@pytest.mark.parametrize("k", SM.KS)
def test_flat_kernel(k, fmt, n, scale):
    pts, designed = flat_points(k, n)
    if n == 4099:
        assert designed.sum() >= (1 << k) + 4  # the whole designed set is in
    L_ref = SM.ref_llr(k, pts, scale).reshape(-1)
    m = M.Modem(cfg(D, mod_type=k), 0)
    d_pts = torch.from_numpy(pts).cuda()
    out = llr_buffer(n * k, fmt)
    m.soft_demap(d_pts, n, out, scale, FMTS[fmt][0])
    torch.cuda.synchronize()
    got = take_llr(out, n * k)
    assert np.array_equal(d_pts.cpu().numpy().view(np.int64), pts.view(np.int64)), "the input was modified"
    what = f"flat k={k} n={n} scale={scale:g}"
    if fmt == "f32":
        SM.check_f32(got, L_ref, scale * 1e-13, what)
    else:
        SM.check_i8(got, L_ref, scale * 1e-13, designed=np.repeat(designed, k), what=what)
        if scale == 64.0 and n >= 63:
            assert (got == 127).any() and (got == -127).any(), "both saturations must occur"
    m.close()


def test_flat_kernel_unaligned_output():
    """An output that is only element aligned takes the element-wise stores."""
    k, n = 6, 4099
    pts, _ = flat_points(k, n)
    m = M.Modem(cfg(D, mod_type=k), 0)
    d_pts = torch.from_numpy(pts).cuda()
    for fmt, off in (("f32", 1), ("i8", 3)):
        L_ref = SM.ref_llr(k, pts, 2.0).reshape(-1)
        buf = llr_buffer(off + n * k, fmt)
        m.soft_demap(d_pts, n, buf[off:], 2.0, FMTS[fmt][0])
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert np.all(h[:off] == SENTINEL)
        got = take_llr(buf[off:], n * k)
        if fmt == "f32":
            SM.check_f32(got, L_ref, 2e-13, "flat unaligned")
        else:
            SM.check_i8(got, L_ref, 2e-13, max_excluded=1.0, what="flat unaligned")
    m.close()


# ------------------------------------------------------------------ fused path: data
FUSED = {**{f"D_k{k}": cfg(D, mod_type=k) for k in SM.KS},
         **{n: ALL_CONFIGS[n] for n in ("D_s12_staged", "D_s1", "D_p16", "D_cp0")}}
LOOP = {n: ALL_CONFIGS[n] for n in ("N64_k1", "N128_k4_s3", "N256_k2")}


@functools.lru_cache(maxsize=None)
def frames(name, nf, stride_extra=0, threads=1):
    """nf frames of config `name`: O.tx_batch + O.awgn at 15 dB. Returns
    (config, payload, iq, frame stride)."""
    p = {**FUSED, **LOOP}[name]
    g = O.geometry(p)
    data = payload(nf * g["bytes_per_frame"], 7)
    stride = g["message_len"] + stride_extra
    x = O.tx_batch(p, data, nf, stride, threads=threads)
    power = float(np.mean(np.abs(x[:g["message_len"]]) ** 2))
    iq = O.awgn(x, np.sqrt(power) * 10 ** (-15 / 20), seed=11, threads=threads)
    return p, data, iq, stride


def channel(p, seed=5):
    rng = np.random.default_rng(seed)
    n = p["num_data_subc"]
    return (1.0 + 0.1 * rng.normal(size=n)) * np.exp(1j * 0.2 * rng.normal(size=n))


def oracle_points(p, iq, nf, stride, chan, threads=1):
    E, _, _ = O.rx_batch(p, iq, nf, stride, threads=threads)
    E = E.reshape(nf, -1)
    if chan is not None:
        E = smith_div(E, np.tile(chan, p["num_symb"])[None, :])
    return E


def run_soft(m, p, iq, nf, stride, fmt, scale, frame_scale=None, chan=None, i16=False, want=("cons", "bytes")):
    """One ofdm_rx_demod_soft launch; returns dict of host arrays."""
    g = O.geometry(p)
    k = p["mod_type"]
    n_llr = nf * g["npts"] * k
    d_iq = torch.from_numpy(iq).cuda()
    llr = llr_buffer(n_llr, fmt)
    cons = torch.zeros((nf * g["npts"],), dtype=torch.complex128, device="cuda") if "cons" in want else None
    out = torch.zeros((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda") if "bytes" in want else None
    d_chan = torch.from_numpy(chan).cuda() if chan is not None else None
    d_fs = torch.from_numpy(frame_scale).cuda() if frame_scale is not None else None
    m.rx_soft(d_iq, nf, llr, scale, FMTS[fmt][0], frame_scale=d_fs, frame_stride=stride, chan=d_chan,
              constell_out=cons, bytes_out=out, i16=i16)
    torch.cuda.synchronize()
    r = {"llr": take_llr(llr, n_llr).reshape(nf, g["npts"], k)}
    if cons is not None:
        r["cons"] = cons.cpu().numpy().reshape(nf, -1)
    if out is not None:
        r["bytes"] = out.cpu().numpy().reshape(nf, -1)
    return r


def check_against_oracle(p, E, r_f32, r_i8, scale, frame_scale, what):
    """Test 3's bars on every frame: both formats against ref_llr(E), and the
    demapper alone against ref_llr of the launch's own constell_out."""
    k = p["mod_type"]
    nf = E.shape[0]
    s_f = scale * (frame_scale if frame_scale is not None else np.ones(nf))
    L_ref = SM.ref_llr(k, E, s_f[:, None])
    bar = (4.0 * s_f * 1e-9 * np.abs(E).max(axis=1))[:, None, None]
    SM.check_f32(r_f32["llr"], L_ref, bar, what + " vs oracle")
    SM.check_i8(r_i8["llr"], L_ref, bar, what=what + " vs oracle")
    for r, fmt in ((r_f32, "f32"), (r_i8, "i8")):
        L_own = SM.ref_llr(k, r["cons"], s_f[:, None])
        tight = (s_f * 1e-13)[:, None, None]
        if fmt == "f32":
            SM.check_f32(r["llr"], L_own, tight, what + " vs own points")
        else:
            SM.check_i8(r["llr"], L_own, tight, what=what + " vs own points")


# ------------------------------------------------------------------ 2. fused vs parent outputs
@pytest.mark.parametrize("inp", ["f64", "i16"])
@pytest.mark.parametrize("with_chan", [False, True])
@pytest.mark.parametrize("name", list(FUSED))
def test_fused_outputs_equal_the_parents(name, with_chan, inp):
    nf = 8
    p, data, iq, stride = frames(name, nf)
    g = O.geometry(p)
    if inp == "i16":
        x = torch.from_numpy(O.get_int16(iq, p["mult"])).cuda()
    else:
        x = torch.from_numpy(iq).cuda()
    chan = torch.from_numpy(channel(p)).cuda() if with_chan else None
    ref = torch.from_numpy(data).cuda()
    m = M.Modem(p, 0)

    def outputs():
        return (torch.zeros((nf * g["npts"],), dtype=torch.complex128, device="cuda"),
                torch.zeros((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda"),
                torch.zeros((1,), dtype=torch.int64, device="cuda"))

    c0, b0, e0 = outputs()
    (m.rx_i16 if inp == "i16" else m.rx)(x, nf, chan=chan, constell_out=c0, bytes_out=b0, ref=ref, bit_errors=e0)
    fmt = "i8" if with_chan else "f32"
    c1, b1, e1 = outputs()
    llr = llr_buffer(nf * g["npts"] * p["mod_type"], fmt)
    m.rx_soft(x, nf, llr, 4.0, FMTS[fmt][0], chan=chan, constell_out=c1, bytes_out=b1, ref=ref, bit_errors=e1,
              i16=inp == "i16")
    torch.cuda.synchronize()
    take_llr(llr, nf * g["npts"] * p["mod_type"])
    assert torch.equal(c0.view(torch.float64).view(torch.int64), c1.view(torch.float64).view(torch.int64))
    assert torch.equal(b0, b1)
    assert int(e0.item()) == int(e1.item())
    m.close()


# ------------------------------------------------------------------ 3. fused vs oracle, 5. consistency
@pytest.mark.parametrize("with_chan", [False, True])
@pytest.mark.parametrize("name", list(FUSED))
def test_fused_llrs_match_the_oracle(name, with_chan):
    nf = 8
    p, data, iq, stride = frames(name, nf)
    k = p["mod_type"]
    chan = channel(p) if with_chan else None
    E = oracle_points(p, iq, nf, stride, chan)
    scale = 8.0
    fs = np.random.default_rng(3).uniform(0.25, 4.0, nf)
    m = M.Modem(p, 0)
    r_f32 = run_soft(m, p, iq, nf, stride, "f32", scale, fs, chan)
    r_i8 = run_soft(m, p, iq, nf, stride, "i8", scale, fs, chan)
    check_against_oracle(p, E, r_f32, r_i8, scale, fs, f"{name} chan={with_chan}")
    # no frame_scale: the scale alone
    r = run_soft(m, p, iq, nf, stride, "f32", scale, None, chan)
    assert np.array_equal(r["cons"].view(np.int64), r_f32["cons"].view(np.int64))
    SM.check_f32(r["llr"], SM.ref_llr(k, r["cons"], scale), scale * 1e-13, f"{name} no frame_scale")
    # 5. away from ties, L < 0 is the bit of the same launch's bytes_out
    g = O.geometry(p)
    bits = np.unpackbits(r_f32["bytes"], axis=1)[:, :g["npts"] * k].reshape(nf, g["npts"], k)
    s_f = (scale * fs)[:, None, None]
    sure = np.abs(r_f32["llr"]) > 1e-6 * s_f
    assert sure.mean() > 0.99
    assert np.array_equal((r_f32["llr"] < 0)[sure], bits[sure] == 1)
    sure8 = np.abs(r_i8["llr"].astype(np.int32)) >= 1
    bits8 = np.unpackbits(r_i8["bytes"], axis=1)[:, :g["npts"] * k].reshape(nf, g["npts"], k)
    assert np.array_equal((r_i8["llr"] < 0)[sure8], bits8[sure8] == 1)
    m.close()


def test_fused_i16_llrs_match_the_oracle():
    """Wire-format input: the LLRs of the exactly converted samples."""
    nf = 8
    p, data, iq, stride = frames("D_k4", nf)
    x16 = O.get_int16(iq, p["mult"])
    w = x16.astype(np.float64)
    iq_conv = w[0::2] + 1j * w[1::2]
    E = oracle_points(p, iq_conv, nf, stride, None)
    m = M.Modem(p, 0)
    r_f32 = run_soft(m, p, x16, nf, stride, "f32", 2.0, i16=True)
    r_i8 = run_soft(m, p, x16, nf, stride, "i8", 2.0, i16=True)
    check_against_oracle(p, E, r_f32, r_i8, 2.0, None, "D_k4 i16")
    m.close()


# ------------------------------------------------------------------ 4. persistent loop
@pytest.mark.parametrize("name,stride_extra,with_chan", [("N64_k1", 0, False), ("N128_k4_s3", 0, True),
                                                         ("N256_k2", 0, False), ("N64_k1", 24, True)])
def test_persistent_loop(name, stride_extra, with_chan):
    """Every workgroup takes at least three frames from the queue."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nf = 3 * 8 * cus + 5
    p, data, iq, stride = frames(name, nf, stride_extra, threads=8)
    chan = channel(p) if with_chan else None
    E = oracle_points(p, iq, nf, stride, chan, threads=8)
    fs = np.random.default_rng(4).uniform(0.25, 4.0, nf)
    m = M.Modem(p, 0)
    r_f32 = run_soft(m, p, iq, nf, stride, "f32", 8.0, fs, chan)
    r_i8 = run_soft(m, p, iq, nf, stride, "i8", 8.0, fs, chan)
    check_against_oracle(p, E, r_f32, r_i8, 8.0, fs, f"{name} x{nf} stride+{stride_extra}")
    assert np.array_equal(r_f32["bytes"], r_i8["bytes"])
    m.close()


# ------------------------------------------------------------------ 6. errors
def test_invalid_arguments():
    nf = 2
    p, data, iq, stride = frames("D_k4", 8)
    g = O.geometry(p)
    m = M.Modem(p, 0)
    L = M.lib()
    d_iq = torch.from_numpy(iq).cuda()
    d_i16 = torch.from_numpy(O.get_int16(iq, p["mult"])).cuda()
    pts = torch.zeros((64,), dtype=torch.complex128, device="cuda")
    llr = torch.zeros((nf * g["npts"] * 4 + 8,), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def flat(points=pts.data_ptr(), scale=1.0, fmt=M.LLR_F32, out=llr.data_ptr()):
        return L.ofdm_soft_demap(m.h, points, 64, scale, fmt, out, st)

    def fused(iq_=d_iq.data_ptr(), iq16=None, scale=1.0, fmt=M.LLR_F32, out=llr.data_ptr()):
        return L.ofdm_rx_demod_soft(m.h, iq_, iq16, nf, stride, None, 0, scale, None, fmt, out, None, None, None,
                                    None, st)

    assert flat() == 0 and fused() == 0 and fused(iq_=None, iq16=d_i16.data_ptr()) == 0
    for call in (flat, fused):
        assert call(out=None) == -1                      # null llr_out
        assert call(fmt=2) == -1 and call(fmt=-1) == -1  # bad fmt
        for s in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
            assert call(scale=s) == -1
        assert call(out=llr.data_ptr() + 2) == -1        # F32 output not 4-byte aligned
        assert call(fmt=M.LLR_I8, out=llr.data_ptr() + 1) == 0  # int8 output: any address
    assert fused(iq_=None, iq16=None) == -1              # neither input
    assert fused(iq16=d_i16.data_ptr()) == -1            # both inputs
    assert flat(points=None) == -1
    torch.cuda.synchronize()
    m.close()


@pytest.mark.parametrize("k", [3, 5, 7])
def test_odd_k_is_unsupported(k):
    """Another k: OFDM_ERR_UNSUPPORTED from the soft entry points. ofdm_create
    itself turns such a modType down (OFDM_ERR_INVALID), so a caller cannot
    hold a context with one: where it does, no soft call can follow."""
    h = C.c_void_p()
    prm = M.Params.make(**cfg(D, mod_type=k))
    rc = M.lib().ofdm_create(C.byref(prm), 0, C.byref(h))
    if rc != 0:
        assert rc == -1
        return
    buf = torch.zeros((64,), dtype=torch.complex128, device="cuda")
    out = torch.zeros((64 * 8,), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert M.lib().ofdm_soft_demap(h, buf.data_ptr(), 64, 1.0, M.LLR_F32, out.data_ptr(), st) == -2
    M.lib().ofdm_destroy(h)
