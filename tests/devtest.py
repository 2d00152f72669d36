"""ctypes binding of c-ofdm_amd/lib/libofdm_devtest.so: test-only launchers
for device primitives no C-ABI entry reaches with chosen arguments
(atan2_fast, cp_phase, unwrap_scan). A missing library is an error."""
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
        for f in (L.ofdm_devtest_atan2, L.ofdm_devtest_cp_phase, L.ofdm_devtest_unwrap):
            f.restype = C.c_int
        _lib = L
    return _lib


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


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
