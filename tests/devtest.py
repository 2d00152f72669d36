"""ctypes binding of c-ofdm_amd/lib/libofdm_devtest.so: test-only launchers
for device primitives no C-ABI entry reaches with chosen arguments
(atan2_fast, cp_phase, unwrap_scan, the pilot windows' first maximum; the
FP64 and packed-FP32 transforms, the
stream walker's T2 sums and screen rule, the FFT preamble search's window
pass), and the longdouble DFT they are compared with. A missing library is an
error."""
import ctypes as C
import os

import numpy as np

# OFDM_DEVTEST_LIB: an alternative build (mutation checks), as OFDM_MI355X_LIB is for the product
LIB_PATH = os.environ.get("OFDM_DEVTEST_LIB") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "c-ofdm_amd", "lib", "libofdm_devtest.so")
UNWRAP_FORMS = [(8, False), (16, False), (64, False), (128, False), (512, False), (64, True)]  # (NT, WAVE)

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `make -C c-ofdm_amd`")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.ofdm_devtest_atan2.argtypes = [vp, vp, vp, C.c_long, vp]
        L.ofdm_devtest_cp_phase.argtypes = [vp, vp, vp, C.c_long, vp]
        L.ofdm_devtest_unwrap.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, C.c_long, vp]
        L.ofdm_devtest_fft64.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, C.c_long, vp]
        L.ofdm_devtest_fft32p.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, C.c_long, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_double, C.c_double, vp]
        L.ofdm_devtest_corr.argtypes = [C.c_int, vp, vp, vp, C.c_long, vp]
        L.ofdm_devtest_window_argmax.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
        for f in (L.ofdm_devtest_atan2, L.ofdm_devtest_cp_phase, L.ofdm_devtest_unwrap, L.ofdm_devtest_fft64,
                  L.ofdm_devtest_fft32p, L.ofdm_devtest_corr, L.ofdm_devtest_window_argmax):
            f.restype = C.c_int
        _lib = L
    return _lib


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # shared references are read-only


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: launcher returned {rc}")


def atan2(y, x) -> np.ndarray:
    """atan2_fast(y, x) elementwise on the device."""
    import torch
    dy, dx = _dev(np.asarray(y, np.float64)), _dev(np.asarray(x, np.float64))
    assert dy.shape == dx.shape and dy.dim() == 1
    out = torch.empty_like(dy)
    _check(lib().ofdm_devtest_atan2(dy.data_ptr(), dx.data_ptr(), out.data_ptr(), dy.numel(), None), "atan2")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def cp_phase(acc, rot) -> np.ndarray:
    """cp_phase(acc, rot) elementwise on the device (complex128 arrays)."""
    import torch
    da, dr = _dev(np.asarray(acc, np.complex128)), _dev(np.asarray(rot, np.complex128))
    assert da.shape == dr.shape and da.dim() == 1
    out = torch.empty((da.numel(),), dtype=torch.float64, device="cuda")
    _check(lib().ofdm_devtest_cp_phase(da.data_ptr(), dr.data_ptr(), out.data_ptr(), da.numel(), None), "cp_phase")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def unwrap(nt: int, wave: bool, seqs) -> list:
    """unwrap_scan<nt, wave> on each sequence of `seqs` (1 <= len <= 4 nt + 1),
    one workgroup per sequence, in one launch. Returns the unwrapped copies."""
    import torch
    stride = 4 * nt + 1
    lens = np.array([len(s) for s in seqs], np.int32)
    assert lens.min() >= 1 and lens.max() <= stride
    buf = np.zeros((len(seqs), stride), np.float64)
    for b, s in enumerate(seqs):
        buf[b, :len(s)] = s
    d, dl = _dev(buf), _dev(lens)
    _check(lib().ofdm_devtest_unwrap(nt, int(wave), d.data_ptr(), dl.data_ptr(), len(seqs), stride, None), "unwrap")
    torch.cuda.synchronize()
    h = d.cpu().numpy()
    return [h[b, :n].copy() for b, n in enumerate(lens)]


def unwrap_serial(ph) -> np.ndarray:
    """The serial one-pass unwrap in float64 (the reference for unwrap())."""
    ph = np.array(ph, np.float64, copy=True)
    pi, two_pi = np.float64(np.pi), np.float64(2 * np.pi)
    for i in range(1, len(ph)):
        d = ph[i] - ph[i - 1]
        if d > pi:
            ph[i] -= two_pi
        elif d < -pi:
            ph[i] += two_pi
    return ph


# ---------------------------------------------------------------- pilot windows
def window_argmax(nt: int, spec, borders):
    """The first maxima of |spec| in the windows [borders[i], borders[i+1]) of
    every row (spec: (n, S) complex128, borders: (n, P + 2) ints within 0..S)
    with a workgroup of nt threads per row. Returns (plain, screened), int32
    (n, P + 1): window_first_max over hypot on every window, and
    window_argmax_screened, which leaves window P/2 alone (-1)."""
    import torch
    spec = np.ascontiguousarray(spec, np.complex128)
    borders = np.ascontiguousarray(borders, np.int32)
    n, S = spec.shape
    P = borders.shape[1] - 2
    assert borders.shape[0] == n and P >= 1 and borders.min() >= 0 and borders.max() <= S
    d, db = _dev(spec), _dev(borders)
    plain = torch.empty((n, P + 1), dtype=torch.int32, device="cuda")
    scr = torch.empty((n, P + 1), dtype=torch.int32, device="cuda")
    _check(lib().ofdm_devtest_window_argmax(nt, d.data_ptr(), db.data_ptr(), P, S, n, plain.data_ptr(),
                                            scr.data_ptr(), None), "window_argmax")
    torch.cuda.synchronize()
    return plain.cpu().numpy(), scr.cpu().numpy()


def window_first_max_model(spec, borders) -> np.ndarray:
    """std::max_element of np.hypot over each window of one spectrum: the first
    maximum; a NaN first element is kept, later NaNs never win; an empty window
    gives its end."""
    mag = np.hypot(np.real(spec), np.imag(spec))
    out = np.empty(len(borders) - 1, np.int32)
    for i, (lo, hi) in enumerate(zip(borders[:-1], borders[1:])):
        if lo >= hi:
            out[i] = hi
        elif np.isnan(mag[lo]):
            out[i] = lo
        else:
            out[i] = lo + int(np.argmax(np.where(np.isnan(mag[lo:hi]), -1.0, mag[lo:hi])))
    return out


def window_first_max_serial(spec, borders) -> np.ndarray:
    """The same by max_element's own loop, one comparison per element."""
    mag = np.hypot(np.real(spec), np.imag(spec))
    out = np.empty(len(borders) - 1, np.int32)
    for i, (lo, hi) in enumerate(zip(borders[:-1], borders[1:])):
        best = lo if lo < hi else hi
        for j in range(lo + 1, hi):
            if mag[best] < mag[j]:
                best = j
        out[i] = best
    return out


# ---------------------------------------------------------------- transforms
FFT_BLOCK, FFT_BLOCK_ACTIVE, FFT_REGS_WAVE = 0, 1, 2
# (form, logn, sign) of every instantiated FP64 transform
FFT64_FORMS = ([(FFT_BLOCK, n, s) for n in range(6, 13) for s in (-1, 1)]
               + [(FFT_BLOCK_ACTIVE, n, -1) for n in range(9, 13)]
               + [(FFT_REGS_WAVE, n, s) for n in range(6, 10) for s in (-1, 1)])
FFT_FORM_NAMES = {FFT_BLOCK: "fft_block", FFT_BLOCK_ACTIVE: "fft_block_active", FFT_REGS_WAVE: "fft_regs_wave"}


def fft64(form: int, logn: int, sign: int, x) -> np.ndarray:
    """The FP64 transform `form` of every row of x (rows of 2^logn complex128),
    one workgroup (or part of a wave) per row, in one launch."""
    import torch
    x = np.ascontiguousarray(x, np.complex128)
    assert x.ndim == 2 and x.shape[1] == 1 << logn
    d = _dev(x)
    out = torch.empty_like(d)
    _check(lib().ofdm_devtest_fft64(form, logn, sign, d.data_ptr(), out.data_ptr(), x.shape[0], None), "fft64")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def fft32p(logt: int, xa, xb, mask=(0, -1, 0, -1), level=0.0, margin=0.0):
    """fft_regs_wave32p<logt, -1> on the block pairs (xa[p], xb[p]) with the
    walker's sums and screen rule. mask = (a1, b1, a2, b2): the detector's two
    bin ranges. Returns (XA, XB complex64, sums float32 (np, 4) = ta, sa, tb,
    sb, verdict int32 (np, 2): 0 certain FAIL, 1 certain PASS, 2 uncertain)."""
    import torch
    xa, xb = np.ascontiguousarray(xa, np.complex128), np.ascontiguousarray(xb, np.complex128)
    assert xa.shape == xb.shape and xa.ndim == 2 and xa.shape[1] == 1 << logt
    n = xa.shape[0]
    da, db = _dev(xa), _dev(xb)
    oa = torch.empty(xa.shape, dtype=torch.complex64, device="cuda")
    ob = torch.empty(xa.shape, dtype=torch.complex64, device="cuda")
    sums = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    verdict = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    a1, b1, a2, b2 = (int(v) for v in mask)
    _check(lib().ofdm_devtest_fft32p(logt, da.data_ptr(), db.data_ptr(), oa.data_ptr(), ob.data_ptr(),
                                     sums.data_ptr(), verdict.data_ptr(), n, a1, b1, a2, b2, float(level),
                                     float(margin), None), "fft32p")
    torch.cuda.synchronize()
    return oa.cpu().numpy(), ob.cpu().numpy(), sums.cpu().numpy(), verdict.cpu().numpy()


def corr(f32: bool, x, H) -> np.ndarray:
    """walk_preamble_fft's window pass on every row of x (512 samples, the
    tail past the window zero) with the spectrum H: IDFT(DFT(x) . H),
    unnormalised (512 times the correlation)."""
    import torch
    x, H = np.ascontiguousarray(x, np.complex128), np.ascontiguousarray(H, np.complex128)
    assert x.ndim == 2 and x.shape[1] == 512 and H.shape == (512,)
    d, dh = _dev(x), _dev(H)
    out = torch.empty_like(d)
    _check(lib().ofdm_devtest_corr(int(f32), d.data_ptr(), dh.data_ptr(), out.data_ptr(), x.shape[0], None), "corr")
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------- the reference transform
LD = np.longdouble
CLD = np.clongdouble
# x87 extended precision (eps 2^-63): 2^10 below FP64's. Elsewhere (longdouble
# = double) the reference falls back to mpmath.
LD_OK = np.finfo(LD).eps <= 2.0 ** -63
_PI_LD = 4 * np.arctan(LD(1))
_tw_cache = {}


def twiddle_ld(n: int, sign: int) -> np.ndarray:
    """e^{sign 2 pi i k / n}, k < n, in the reference precision."""
    key = (n, sign)
    if key not in _tw_cache:
        if LD_OK:
            a = 2 * _PI_LD * np.arange(n, dtype=LD) / LD(n)
            w = np.cos(a) + 1j * (sign * np.sin(a))
        else:
            import mpmath
            mpmath.mp.dps = 40
            w = np.array([complex(mpmath.expjpi(mpmath.mpf(2 * sign * k) / n)) for k in range(n)], CLD)
        _tw_cache[key] = w.astype(CLD)
    return _tw_cache[key]


def dft_ref(x, sign: int = -1) -> np.ndarray:
    """Unnormalised DFT along the last axis (a power of two) in longdouble:
    radix-2 recursion, twiddles evaluated directly at each level."""
    x = np.asarray(x).astype(CLD)
    if not LD_OK:
        return _dft_mp(x, sign)
    n = x.shape[-1]
    if n == 1:
        return x
    e, o = dft_ref(x[..., 0::2], sign), dft_ref(x[..., 1::2], sign)
    o = o * twiddle_ld(n, sign)[: n // 2]
    return np.concatenate([e + o, e - o], axis=-1)


def _dft_mp(x, sign):
    import mpmath
    mpmath.mp.dps = 40
    n = x.shape[-1]
    w = [mpmath.expjpi(mpmath.mpf(2 * sign * k) / n) for k in range(n)]
    flat = x.reshape(-1, n)
    out = np.empty(flat.shape, CLD)
    for r, row in enumerate(flat):
        v = [mpmath.mpc(float(z.real), float(z.imag)) for z in row]
        out[r] = [complex(mpmath.fsum(v[j] * w[(j * k) % n] for j in range(n))) for k in range(n)]
    return out.reshape(x.shape)


def impulse_dft(n: int, idx, sign: int, ampl=1.0) -> np.ndarray:
    """The DFT of ampl * delta[j - idx] in closed form: ampl e^{sign 2 pi i idx k / n}."""
    idx = np.asarray(idx, np.int64)
    k = np.arange(n, dtype=np.int64)
    return LD(ampl) * twiddle_ld(n, sign)[(idx[:, None] * k[None, :]) % n]


def rel_l2(got, ref) -> np.ndarray:
    """||got - ref||_2 / ||ref||_2 per row, in the reference precision."""
    d = np.asarray(got).astype(CLD) - ref
    num = np.sqrt(np.sum(d.real ** 2 + d.imag ** 2, axis=-1))
    den = np.sqrt(np.sum(ref.real ** 2 + ref.imag ** 2, axis=-1))
    return (num / den).astype(np.float64)


def t2_mask(n: int, mask) -> np.ndarray:
    """The detector's bin weights (0, 1 or 2) of the ranges (a1, b1, a2, b2)."""
    a1, b1, a2, b2 = mask
    k = np.arange(n)
    return ((k >= a1) & (k <= b1)).astype(np.int64) + ((k >= a2) & (k <= b2)).astype(np.int64)


def t2_ratio_ref(x, mask) -> np.ndarray:
    """The detector ratio sum_k m_k |X_k|^2 / sum_k |X_k|^2 of every row in longdouble."""
    X = dft_ref(x, -1)
    e = X.real ** 2 + X.imag ** 2
    return np.sum(e * t2_mask(x.shape[-1], mask).astype(LD), axis=-1) / np.sum(e, axis=-1)
