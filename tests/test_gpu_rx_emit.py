"""The rx emit's fast path (k = 2 without a channel, D a multiple of 64,
word-aligned outputs): decisions as threshold compares and output words
assembled inside the wave, against the path it replaces. The device helpers
cover k = 4 as well and are tested for it; the kernel keeps 16-QAM on the
old path (no measured gain), so its k = 4 cases check that path unchanged.

1. decide_tau (thresholds found by the context's scan) equals decide_select
   bit for bit on the doubles around every threshold and nominal edge, the
   special values and 10^6 random points.
2. emit_words (the in-wave byte assembly) equals pack_word's byte layout.
3. The whole kernel: the same noisy IQ through rx with aligned outputs (fast
   path) and with bytes_out / ref at a 1-byte offset (the byte-wise path):
   bytes, bit errors and constellation identical, and equal to the oracle.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from common import B, D, cfg, payload, rel_err
from devtest import LIB_PATH

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

_lib = None


def dlib():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.ofdm_devtest_tau_scan.argtypes = [C.c_int, vp, vp]
        L.ofdm_devtest_decide.argtypes = [C.c_int, vp, vp, vp, vp, C.c_long, vp]
        L.ofdm_devtest_emit_words.argtypes = [C.c_int, vp, vp, C.c_int, vp]
        for f in (L.ofdm_devtest_tau_scan, L.ofdm_devtest_decide, L.ofdm_devtest_emit_words):
            f.restype = C.c_int
        _lib = L
    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def scan(k):
    out = torch.zeros((4,), dtype=torch.float64, device="cuda")
    assert dlib().ofdm_devtest_tau_scan(k, out.data_ptr(), None) == 0
    h = host(out)
    return h[:3], h[3]


def key(x):
    """Order-preserving int64 key of a float64 (adjacent doubles, adjacent keys)."""
    b = np.asarray(x, np.float64).view(np.int64)
    return b ^ ((b >> 63) & np.int64(0x7FFFFFFFFFFFFFFF))


def unkey(k):
    k = np.asarray(k, np.int64)
    return (k ^ ((k >> 63) & np.int64(0x7FFFFFFFFFFFFFFF))).view(np.float64)


@pytest.mark.parametrize("k", [2, 4])
def test_threshold_decision_equals_decide_select(k):
    m = 1 << (k // 2)
    tau, verdict = scan(k)
    assert verdict == 1.0, "the scan's own checks failed"
    tau = tau[:m - 1]
    edges = np.array([-1.0 + (2 * j - 1) / (m - 1) for j in range(1, m)])
    assert np.all(np.isfinite(tau)) and np.all(np.diff(tau) > 0)
    assert np.all(np.abs(tau - edges) < 2e-15), (tau, edges)  # three roundings of values below 4: 3 x 4.4e-16
    eps = np.finfo(np.float64).eps
    around = np.concatenate([unkey(key(c) + np.arange(-64, 65)) for c in np.concatenate([tau, edges])])
    special = np.array([0.0, -0.0, 1.0, -1.0, 1.0 + eps, 1.0 - eps / 2, -1.0 - eps, -1.0 + eps / 2,
                        2.0, -2.0, np.inf, -np.inf, np.nan])
    rnd = np.random.default_rng(k).uniform(-1.5, 1.5, 1_000_000)
    v = np.concatenate([around, special, rnd])
    # every value on each axis, against varied values on the other
    def cplx(re, im):
        z = np.empty(np.broadcast(re, im).shape, np.complex128)
        z.real, z.imag = re, im
        return z.ravel()

    z = np.concatenate([cplx(v, np.roll(v, 7)), cplx(np.roll(v, 3), v), cplx(special[:, None], special[None, :])])
    dz, dt = dev(z), dev(np.concatenate([tau, np.full(3 - len(tau), np.inf)]))
    sel = torch.full((len(z),), 255, dtype=torch.uint8, device="cuda")
    thr = torch.full((len(z),), 254, dtype=torch.uint8, device="cuda")
    assert dlib().ofdm_devtest_decide(k, dz.data_ptr(), dt.data_ptr(), sel.data_ptr(), thr.data_ptr(), len(z),
                                      None) == 0
    hs, ht = host(sel), host(thr)
    bad = np.nonzero(hs != ht)[0]
    assert bad.size == 0, f"{bad.size} mismatches, first z = {z[bad[:4]]}: {hs[bad[:4]]} vs {ht[bad[:4]]}"
    assert hs.max() < (1 << k)
    # the levels are all exercised
    assert set(np.unique(hs[:len(v)])) == set(range(1 << k))


@pytest.mark.parametrize("k", [2, 4])
def test_emit_words_layout(k):
    """emit_words against pack_word's layout: byte j of a group holds carriers
    LPB j .. LPB j + LPB - 1, the first in the top bits."""
    lpb, nw = 8 // k, 5
    rng = np.random.default_rng(10 + k)
    dec = rng.integers(0, 1 << k, (nw, 4, 64), dtype=np.uint32)  # wave, group, lane
    dec[0] = (1 << k) - 1
    dec[1] = np.arange(64)[None, :] % (1 << k)
    bits = (dec[:, 0] | (dec[:, 1] << 8) | (dec[:, 2] << 16) | (dec[:, 3] << 24)).astype(np.uint32)
    words = torch.zeros((nw * 64 * 2,), dtype=torch.int32, device="cuda")
    assert dlib().ofdm_devtest_emit_words(k, dev(bits.view(np.int32)).data_ptr(), words.data_ptr(), nw, None) == 0
    got = host(words).view(np.uint32).reshape(nw, 64, 2)
    # the model: the bytes of each group, as little-endian words
    by = np.zeros((nw, 4, 64 // lpb), np.uint32)
    for r in range(lpb):
        by = (by << k) | dec[:, :, r::lpb]
    want = by[..., 0::4] | (by[..., 1::4] << 8) | (by[..., 2::4] << 16) | (by[..., 3::4] << 24)
    seen = np.zeros(want.shape, bool)
    for lane in range(64):
        if ((lane // lpb) & 3) != 3:
            continue
        for h in range(k // 2):
            g, wi = (lane & (lpb - 1)) + lpb * h, lane // (4 * lpb)
            assert np.array_equal(got[:, lane, h], want[:, g, wi]), (lane, h)
            seen[:, g, wi] = True
    assert seen.all()  # the collecting lanes cover every word of every group


# (name, config, frames): nframes > 128 keeps a config whose frame fits one
# workgroup (S * N/8 <= 1024 threads) on the persistent kernel under test.
# The persistent grid is capped at 8 waves per CU (rx_launch_n): 8 workgroups
# per CU at N = 512 (T = 64), 2 at N = 2048 (T = 256). A frame count given as
# (workgroups per CU, extra) stands for 3 x that cap + extra frames, so every
# workgroup takes a second and a third frame from the queue: the reference
# bytes' DMA into the FFT image, the next frame's symbol-0 DMA in flight
# during the emit, and the frame-end barrier are exercised across frames.
N512 = cfg(D, mod_type=2)
N1024 = cfg(D, fft_size=1024, num_data_subc=448, num_pilot_subc=16, cp_size=256)
CASES = [
    ("N512-k2-queue", N512, (8, 5)),
    ("B-queue", B, (2, 5)),  # the headline geometry over several frames per workgroup
    ("N512-k4", cfg(N512, mod_type=4), 130),
    ("N512-D128-k2", cfg(N512, num_data_subc=128), 130),
    ("N512-D128-k4-S3", cfg(N512, num_data_subc=128, mod_type=4, num_symb=3), 130),
    ("N1024-D448-k2", cfg(N1024, mod_type=2), 130),
    ("N1024-D448-k4", cfg(N1024, mod_type=4), 130),
    ("B-3frames", B, 3),
    ("B-1frame", B, 1),
    ("B-k4-3frames", cfg(B, mod_type=4), 3),
    ("B-S1", cfg(B, num_symb=1), 130),
    ("B-S3", cfg(B, num_symb=3), 130),
    ("N512-D200-k6-fallback", cfg(N512, num_data_subc=200, mod_type=6), 130),
]


@pytest.mark.parametrize("name,c,nf", CASES, ids=[x[0] for x in CASES])
def test_fast_path_equals_bytewise_path_and_oracle(name, c, nf):
    if isinstance(nf, tuple):
        nf = 3 * nf[0] * torch.cuda.get_device_properties(0).multi_processor_count + nf[1]
    m = M.Modem(c, 0)
    # the context offers the new emit exactly where the kernel is built for it
    # (a failed threshold scan would quietly leave both runs on the old code)
    assert m.rx_emit_fast() == (c["mod_type"] == 2)
    g = O.geometry(c)
    bpf, npf, msg = g["bytes_per_frame"], g["npts"], g["message_len"]
    data = payload(nf * bpf, seed=len(name))
    ref = payload(nf * bpf, seed=1 + len(name))  # not the payload: many bit errors to count
    clean = O.tx_batch(c, data, nf, threads=8)
    es = np.mean(np.abs(O.constellation(c["mod_type"])) ** 2)
    for snr_db in (10.0, 0.0):
        iq = O.awgn(clean, np.sqrt(es / 10 ** (snr_db / 10)), seed=int(snr_db) + 5, threads=8)
        ocons, obytes, oerrs = O.rx_batch(c, iq, nf, msg, ref=ref, threads=8)
        d_iq = dev(iq)
        res = []
        for off in (0, 1):
            cons = torch.full((nf * npf,), np.nan, dtype=torch.complex128, device="cuda")
            out = torch.full((nf * bpf + 8,), 0xA5, dtype=torch.uint8, device="cuda")
            rbuf = torch.zeros((nf * bpf + 8,), dtype=torch.uint8, device="cuda")
            rbuf[off:off + nf * bpf] = dev(ref)
            errs = torch.zeros((1,), dtype=torch.int64, device="cuda")
            assert (out.data_ptr() + off) % 4 == off
            m.rx(d_iq, nf, constell_out=cons, bytes_out=out[off:], ref=rbuf[off:], bit_errors=errs)
            ho = host(out)
            assert np.all(ho[:off] == 0xA5) and np.all(ho[off + nf * bpf:] == 0xA5), "wrote outside the frames"
            res.append((ho[off:off + nf * bpf], int(host(errs)[0]), host(cons)))
        (b0, e0, c0), (b1, e1, c1) = res
        assert np.array_equal(b0, b1), (name, snr_db)
        assert e0 == e1
        assert np.array_equal(c0.view(np.uint64), c1.view(np.uint64)), "constellation not bit-identical"
        assert np.array_equal(b0, obytes), (name, snr_db)
        assert e0 == oerrs > 0
        assert rel_err(c0, ocons) < 1e-10
    # bytes only, no constellation and no reference: the stores' own branches
    out = torch.zeros((nf * bpf,), dtype=torch.uint8, device="cuda")
    m.rx(d_iq, nf, bytes_out=out)
    assert np.array_equal(host(out), obytes)
    m.close()
