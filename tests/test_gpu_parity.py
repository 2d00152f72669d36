"""GPU parity: the HIP path (through the C-ABI) against the oracle on the same
seeded inputs, against the reference's golden files, and — at BASELINE.json's
full size — through size-independent properties (loopback round trip, BER).

Tolerances (BASELINE.json north_star): demod decisions / bytes / int16 wire
samples bit-exact; complex IQ and constellation within 1e-6 relative (we
assert 1e-10: both sides are FP64 and differ only by FFT rounding order).
"""
import numpy as np
import pytest

import oracle as O
from common import ALL_CONFIGS, B, CC, G, assert_int16_match, golden, payload, rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

TOL = 1e-10
_modems = {}


def modem(name_or_cfg):
    key = name_or_cfg if isinstance(name_or_cfg, str) else repr(sorted(name_or_cfg.items()))
    if key not in _modems:
        cfg = ALL_CONFIGS[name_or_cfg] if isinstance(name_or_cfg, str) else name_or_cfg
        _modems[key] = M.Modem(cfg, 0)
    return _modems[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


NFR = {"B": 3, "C": 2}
CFGS = sorted(ALL_CONFIGS)


@pytest.mark.parametrize("name", CFGS)
def test_tx_matches_oracle(name):
    cfg = ALL_CONFIGS[name]
    m = modem(name)
    g = O.geometry(cfg)
    nf = NFR.get(name, 4)
    data = payload(nf * g["bytes_per_frame"], seed=hash(name) & 0xFFFF)
    stride = g["message_len"] + 7  # non-contiguous frames
    iq = torch.full((nf * stride,), complex(9.0, 9.0), dtype=torch.complex128, device="cuda")
    iq16 = torch.zeros((nf * stride * 2,), dtype=torch.int16, device="cuda")
    m.tx(dev(data), nf, iq, frame_stride=stride, iq16_out=iq16)
    got = host(iq).reshape(nf, stride)
    got16 = host(iq16).reshape(nf, stride * 2)
    ref = O.tx_batch(cfg, data, nf, stride).copy()
    ref = np.concatenate([ref, np.zeros(nf * stride - len(ref), np.complex128)]).reshape(nf, stride)
    L = g["message_len"]
    assert rel_err(got[:, :L], ref[:, :L]) < TOL
    assert np.all(got[:, L:] == complex(9.0, 9.0)), "gap between frames must be untouched"
    assert_int16_match(got16[:, : 2 * L], ref[:, :L], cfg["mult"])


def test_tx_frames_regenerate_source_bin():
    gd = golden()
    m = modem("G")
    g = O.geometry(G)
    fr = torch.zeros((g["frame_len"],), dtype=torch.complex128, device="cuda")
    fr16 = torch.zeros((2 * g["frame_len"],), dtype=torch.int16, device="cuda")
    m.tx_frames(dev(gd["payload"]), 1, fr, fr16)
    assert np.array_equal(host(fr16), gd["source"])  # reference data/source.bin, bit-exact
    assert rel_err(host(fr), O.frame_write(G, gd["payload"])) < TOL
    # constants exposed for FRAME_FORM::preamble / t2sin
    b, pre, modp, tpl = m.preamble()
    assert list(b) == gd["preamble_bytes"]
    opre, omodp, otpl = O.preamble_setup(G)
    assert rel_err(pre, opre) < TOL and np.array_equal(modp, omodp) and rel_err(tpl, otpl) < TOL
    assert rel_err(m.t2_symbol(), O.t2_symbol(G)) < TOL


@pytest.mark.parametrize("name", CFGS)
@pytest.mark.parametrize("snr_db", [None, 12.0])
def test_rx_matches_oracle(name, snr_db):
    cfg = ALL_CONFIGS[name]
    m = modem(name)
    g = O.geometry(cfg)
    nf = NFR.get(name, 4)
    data = payload(nf * g["bytes_per_frame"], seed=7 + len(name))
    stride = g["message_len"] + 3
    iq = O.tx_batch(cfg, data, nf, stride)
    iq = np.concatenate([iq, np.zeros(nf * stride - len(iq), np.complex128)])
    if snr_db is not None:
        es = np.mean(np.abs(O.constellation(cfg["mod_type"])) ** 2)
        iq = O.awgn(iq, np.sqrt(es / 10 ** (snr_db / 10)), seed=99)
    cons = torch.zeros((nf * g["npts"],), dtype=torch.complex128, device="cuda")
    out = torch.zeros((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
    errs = torch.zeros((1,), dtype=torch.int64, device="cuda")
    m.rx(dev(iq), nf, frame_stride=stride, constell_out=cons, bytes_out=out, ref=dev(data), bit_errors=errs)
    ocons, obytes, oerrs = O.rx_batch(cfg, iq, nf, stride, ref=data)
    assert rel_err(host(cons), ocons) < TOL
    assert np.array_equal(host(out), obytes)
    assert int(host(errs)[0]) == oerrs
    if snr_db is None:
        assert oerrs == 0 and np.array_equal(obytes, data)


def test_rx_bytes_only_and_constell_only():
    cfg = B
    m = modem("B")
    g = O.geometry(cfg)
    nf = 5
    data = payload(nf * g["bytes_per_frame"], seed=3)
    iq = O.awgn(O.tx_batch(cfg, data, nf), 0.3, seed=5)
    ocons, obytes, _ = O.rx_batch(cfg, iq, nf, g["message_len"])
    out = torch.zeros((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
    m.rx(dev(iq), nf, bytes_out=out)
    assert np.array_equal(host(out), obytes)
    cons = torch.zeros((nf * g["npts"],), dtype=torch.complex128, device="cuda")
    m.rx(dev(iq), nf, constell_out=cons)
    assert rel_err(host(cons), ocons) < TOL


def test_rx_golden_capture_with_channel_estimate():
    """data/constell.bin: the reference's equalised constellation of frame 1,
    fed through the GPU rx with the golden chan_char_lq divisor (main.cpp:66-71)."""
    gd = golden()
    g = O.geometry(G)
    x = gd["data"]
    pr = gd["preamble_begin"][0]
    mwp = x[pr: pr + g["preamble_len"] + g["message_len"]].copy()
    pre, modp, _ = O.preamble_setup(G)
    mwp = O.freq_shift(mwp, gd["cfo_frame1"])
    mwp = O.cp_freq_sinh(G, mwp)
    mwp = O.pr_phase_sinh(mwp, pre)
    msg = np.ascontiguousarray(mwp[g["preamble_len"]:])
    m = modem("G")
    cons = torch.zeros((g["npts"],), dtype=torch.complex128, device="cuda")
    out = torch.zeros((g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
    m.rx(dev(msg), 1, chan=dev(gd["phases"]), constell_out=cons, bytes_out=out)
    assert rel_err(host(cons), gd["constell"]) < 1e-6
    assert np.abs(host(cons) - gd["constell"]).max() < 1e-12
    assert np.array_equal(host(out), gd["payload"])


def test_rx_demod_read_one_launch_equals_rx_with_and_without_channel():
    """ofdm_rx_demod_read (the drop-in's run-ahead of rx.cpp:211-220): its
    read_out equals rx without a divisor (FFT_FORM::read), its points and
    bytes equal rx with the divisor, bit for bit; outputs in device memory or
    written straight into page-locked host memory alike."""
    cfg = CC
    m = modem("C")
    g = O.geometry(cfg)
    nf, D = 3, cfg["num_data_subc"]
    data = payload(nf * g["bytes_per_frame"], seed=21)
    iq = dev(O.awgn(O.tx_batch(cfg, data, nf), 0.05, seed=22))
    rng = np.random.default_rng(23)
    chan = dev(np.exp(1j * rng.uniform(-0.3, 0.3, nf * D)) * rng.uniform(0.8, 1.2, nf * D))
    npts = nf * g["npts"]
    read0 = torch.zeros((npts,), dtype=torch.complex128, device="cuda")
    m.rx(iq, nf, constell_out=read0)
    cons1 = torch.zeros((npts,), dtype=torch.complex128, device="cuda")
    out1 = torch.zeros((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
    m.rx(iq, nf, chan=chan, chan_stride=D, constell_out=cons1, bytes_out=out1)
    for pinned in (False, True):
        kw = {"dtype": torch.complex128}
        read = torch.zeros((npts,), **kw, pin_memory=True) if pinned else torch.zeros((npts,), **kw, device="cuda")
        cons = torch.zeros((npts,), **kw, pin_memory=True) if pinned else torch.zeros((npts,), **kw, device="cuda")
        out = (torch.zeros((nf * g["bytes_per_frame"],), dtype=torch.uint8, pin_memory=True) if pinned else
               torch.zeros((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda"))
        m.rx_read(iq, nf, chan, read, chan_stride=D, constell_out=cons, bytes_out=out)
        torch.cuda.synchronize()
        assert torch.equal(read.cpu(), read0.cpu())
        assert torch.equal(cons.cpu(), cons1.cpu())
        assert torch.equal(out.cpu(), out1.cpu())
    # the division is the reference's (libgcc Smith division, main.cpp:69-71)
    c = host(cons1).reshape(nf, -1)
    want = host(read0).reshape(nf, -1) / np.tile(host(chan).reshape(nf, D), (1, g["npts"] // D))
    assert rel_err(c, want) < 1e-14


WIDE = ["D", "D_cp0", "D_p2", "D_p16", "D_qam256", "D_qam64", "D_qpsk", "D_s1", "G"]


@pytest.mark.parametrize("name", WIDE)
def test_few_frame_rx_equals_persistent_rx(name):
    """rx on a few frames (one workgroup per frame, a wave per symbol: the
    drop-in's one-frame calls) equals the persistent one-wave-per-frame rx
    that a large batch takes, bit for bit: points, bytes, bit errors, with
    and without a channel divisor, and rx_demod_read's pre-division points."""
    cfg = ALL_CONFIGS[name]
    m = modem(name)
    g = O.geometry(cfg)
    nf, D, bpf, npf = 300, cfg["num_data_subc"], g["bytes_per_frame"], g["npts"]
    data = torch.from_numpy(payload(nf * bpf, seed=31)).cuda()
    iq = torch.zeros((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
    m.tx(data, nf, iq, noise_std=0.3, seed=32)
    rng = np.random.default_rng(33)
    chan = dev(np.exp(1j * rng.uniform(-0.3, 0.3, nf * D)) * rng.uniform(0.8, 1.2, nf * D))
    ref = torch.from_numpy(payload(nf * bpf, seed=34)).cuda()

    def run(lo, hi, c, outs):
        cons, byt, rd, errs = outs
        k = hi - lo
        msg = iq[lo * g["message_len"]:]
        if c is None:
            m.rx(msg, k, constell_out=cons[lo * npf:], bytes_out=byt[lo * bpf:], ref=ref[lo * bpf:], bit_errors=errs)
        else:
            m.rx_read(msg, k, c[lo * D:], rd[lo * npf:], chan_stride=D, constell_out=cons[lo * npf:],
                      bytes_out=byt[lo * bpf:])

    def outs():
        return (torch.full((nf * npf,), np.nan, dtype=torch.complex128, device="cuda"),
                torch.zeros((nf * bpf,), dtype=torch.uint8, device="cuda"),
                torch.full((nf * npf,), np.nan, dtype=torch.complex128, device="cuda"),
                torch.zeros((1,), dtype=torch.int64, device="cuda"))

    for c in (None, chan):
        big, few = outs(), outs()
        run(0, nf, c, big)
        for lo in range(0, nf, 7):
            run(lo, min(nf, lo + 7), c, few)
        torch.cuda.synchronize()
        for a, b in zip(big, few):
            if c is not None or a is not big[2]:
                assert torch.equal(a.cpu(), b.cpu()), name
    # and the oracle on a frame
    f = 5
    oc = O.ofdm_fft(cfg, host(iq)[f * g["message_len"]:(f + 1) * g["message_len"]])
    assert rel_err(host(few[0])[f * npf:(f + 1) * npf] * np.tile(host(chan)[f * D:(f + 1) * D], cfg["num_symb"]),
                   oc) < 1e-9


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096, 100003])
def test_copy_kernel_device_and_pinned(n):
    """ofdm_copy: device <-> device / page-locked host, aligned (16-B body +
    tail) and misaligned (byte) forms."""
    m = modem("D")
    src = torch.randint(0, 256, (n + 64,), dtype=torch.uint8, device="cuda")
    for off_s, off_d in ((0, 0), (16, 32), (3, 5)):
        want = src[off_s:off_s + n].cpu()
        d = torch.zeros((n + 64,), dtype=torch.uint8, device="cuda")
        m.copy(d[off_d:], src[off_s:], n)
        h = torch.zeros((n + 64,), dtype=torch.uint8, pin_memory=True)
        m.copy(h[off_d:], src[off_s:], n)
        back = torch.zeros((n + 64,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        m.copy(back[off_d:], h[off_d:], n)
        torch.cuda.synchronize()
        assert torch.equal(d[off_d:off_d + n].cpu(), want)
        assert torch.equal(h[off_d:off_d + n], want)
        assert torch.equal(back[off_d:off_d + n].cpu(), want)
        assert int(d[:off_d].sum()) == 0 and int(d[off_d + n:].sum()) == 0  # nothing past the range


@pytest.mark.parametrize("k", [1, 2, 4, 6, 8])
def test_demap_and_map_match_oracle(k):
    cfg = dict(ALL_CONFIGS["D"], mod_type=k)
    m = modem(cfg)
    rng = np.random.default_rng(k)
    n = 1000 + k
    pts = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.8
    pts[:3] = [0.0, 1.0 / 3.0 + 1j, -3.0 - 3j]
    t = dev(pts)
    nb = (n * k + 7) // 8
    out = torch.zeros((nb,), dtype=torch.uint8, device="cuda")
    m.demap(t, n, out)
    ob, opts = O.demod(k, pts)
    assert np.array_equal(host(out), ob)
    assert np.array_equal(host(t), opts)  # clamped in place, like Modulation::demod
    data = payload(333, seed=k)
    npts = (333 * 8 + k - 1) // k
    pts_out = torch.zeros((npts,), dtype=torch.complex128, device="cuda")
    m.map(dev(data), 333, pts_out)
    assert np.array_equal(host(pts_out), O.mod(k, data))


def test_full_size_loopback_config_b():
    """BASELINE config 2 at full size (65 536 symbols = 8 192 frames): tx then rx
    on the GPU; clean channel decodes every byte, AWGN BER is in the expected band,
    and a sample of frames equals the oracle on the same noisy samples."""
    m = modem("B")
    g = O.geometry(B)
    nf = 8192
    data = payload(nf * g["bytes_per_frame"], seed=2024)
    d_data = dev(data)
    iq = torch.empty((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
    out = torch.empty((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
    errs = torch.zeros((1,), dtype=torch.int64, device="cuda")
    m.tx(d_data, nf, iq)
    m.rx(iq, nf, bytes_out=out, ref=d_data, bit_errors=errs)
    assert int(host(errs)[0]) == 0
    assert torch.equal(out, d_data)
    # Es/N0 = 10 dB QPSK (constellation energy 2)
    errs.zero_()
    m.tx(d_data, nf, iq, noise_std=float(np.sqrt(2.0 / 10.0)), seed=11)
    m.rx(iq, nf, bytes_out=out, ref=d_data, bit_errors=errs)
    ber = int(host(errs)[0]) / (8.0 * len(data))
    assert 3e-4 < ber < 5e-3, ber
    idx = [0, 1, 4095, 8191]
    h = host(iq).reshape(nf, g["message_len"])
    hb = host(out).reshape(nf, -1)
    for f in idx:
        _, ob, _ = O.rx_batch(B, h[f], 1, g["message_len"])
        assert np.array_equal(ob, hb[f])
    # the GPU noise equals the oracle's counter-based noise
    clean = O.tx_batch(B, data[: g["bytes_per_frame"]], 1)
    noisy = O.awgn(clean, float(np.sqrt(2.0 / 10.0)), seed=11)
    # the channel model's tolerance, on the noise component: the GPU's FP32
    # Box-Muller transcendentals against the oracle's FP64 draw of the same
    # counters (measured ~1e-7)
    assert rel_err(h[0] - clean, noisy - clean) < 1e-6


def test_awgn_counter_crosses_2_32_boundary():
    """The fused channel noise is a function of (seed, global sample index) only:
    frames whose sample counter wraps the low 32-bit word, with a seed using its
    high word, match the oracle's counter definition (orc_awgn)."""
    m = modem("B")
    g = O.geometry(B)
    nf = 3
    data = payload(nf * g["bytes_per_frame"], seed=31)
    off = (1 << 32) - g["message_len"] - 777  # frame 1 holds the wrap
    seed = (7 << 40) + 12345
    iq = torch.empty((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
    m.tx(dev(data), nf, iq, noise_std=0.3, seed=seed, sample_offset=off)
    clean = O.tx_batch(B, data, nf)
    want = O.awgn(clean, 0.3, seed=seed, sample_offset=off)
    got = host(iq)
    assert rel_err(got - clean, want - clean) < 1e-6  # the channel model's tolerance on the noise


def test_full_size_config_c_roundtrip():
    m = modem("C")
    g = O.geometry(CC)
    nf = 2048
    data = payload(nf * g["bytes_per_frame"], seed=77)
    d = dev(data)
    iq = torch.empty((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
    out = torch.empty_like(d)
    m.tx(d, nf, iq)
    m.rx(iq, nf, bytes_out=out)
    assert torch.equal(out, d)


def test_invalid_arguments_raise():
    m = modem("D")
    g = O.geometry(ALL_CONFIGS["D"])
    iq = torch.zeros((g["message_len"],), dtype=torch.complex128, device="cuda")
    with pytest.raises(M.OfdmError):
        m.rx(iq, 1, frame_stride=g["message_len"] - 1)
    with pytest.raises(M.OfdmError):
        M.Modem(dict(ALL_CONFIGS["D"], fft_size=500))
    with pytest.raises(M.OfdmError):
        M.Modem(dict(ALL_CONFIGS["D"], mod_type=3))


@pytest.mark.parametrize("name", ["D", "B", "N64_k1", "D_s12_staged"])
def test_fft_form_write_read_match_oracle(name):
    """FFT_FORM::write / ::read (Frame.cpp:54-96) on FFT_buf layouts."""
    cfg = ALL_CONFIGS[name]
    m = modem(name)
    N, D, P, S = cfg["fft_size"], cfg["num_data_subc"], cfg["num_pilot_subc"], cfg["num_symb"]
    ampl = cfg["pilot_ampl"] / 1000
    nf = 3
    rng = np.random.default_rng(4)
    pts = O.constellation(cfg["mod_type"])[rng.integers(0, 1 << cfg["mod_type"], nf * D * S)]
    fb = torch.zeros((nf * N * S,), dtype=torch.complex128, device="cuda")
    m.fft_write(dev(pts), nf, fb)
    ref_fb = np.concatenate([(lambda o: (O.lib().orc_fft_write(N, D, P, S, ampl, O._d(pts[f * D * S:(f + 1) * D * S].copy()), O._d(o)), o)[1])(np.zeros(N * S, np.complex128)) for f in range(nf)])
    assert rel_err(host(fb), ref_fb) < TOL
    noisy = O.awgn(ref_fb, 0.05, seed=3)
    rest = torch.zeros((nf * D * S,), dtype=torch.complex128, device="cuda")
    m.fft_read(dev(noisy), nf, rest)
    want = []
    for f in range(nf):
        buf = noisy[f * N * S:(f + 1) * N * S].copy()
        o = np.zeros(D * S, np.complex128)
        O.lib().orc_fft_read(N, D, P, S, ampl, O._d(buf), O._d(o))
        want.append(o)
    assert rel_err(host(rest), np.concatenate(want)) < TOL


@pytest.mark.parametrize("ib,ob", [(8, 1), (8, 2), (8, 4), (8, 6), (8, 8), (1, 8), (2, 8), (4, 8), (6, 8), (3, 5)])
def test_bit_convert_matches_oracle(ib, ob):
    m = modem("D")
    rng = np.random.default_rng(ib * 10 + ob)
    for n in (1, 7, 1000):
        data = rng.integers(0, 1 << ib, n, dtype=np.uint8)
        out = torch.zeros((n * 8 + 8,), dtype=torch.uint8, device="cuda")
        k = m.bit_convert(dev(data), n, ib, ob, out)
        want = O.bit_convert(ob, ib, data)
        assert k == len(want)
        assert np.array_equal(host(out)[:k], want)


def test_int16_to_double():
    m = modem("D")
    v = np.random.default_rng(0).integers(-32768, 32767, 2 * 10007, dtype=np.int16)
    out = torch.zeros((10007,), dtype=torch.complex128, device="cuda")
    m.int16_to_double(dev(v), 10007, out)
    h = host(out)
    assert np.array_equal(h.real, v[0::2].astype(np.float64)) and np.array_equal(h.imag, v[1::2].astype(np.float64))


def test_config3_ber_sweep_points_match_oracle():
    """SURVEY §8d config 3 (C, 16-QAM, AWGN at Es/N0 with seed 1000+SNR): at
    sampled SNRs the GPU's decisions on the noisy IQ equal the oracle's bit for
    bit, the BER falls with SNR, and the GPU noise equals the oracle's
    counter-based noise."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "ber_sweep", os.path.join(os.path.dirname(__file__), "..", "tools", "ber_sweep.py"))
    bs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bs)
    m = modem("C")
    g = O.geometry(CC)
    rows = bs.sweep(m, CC, [4.0, 10.0, 16.0], 3e5, torch)
    bers = [r["ber"] for r in rows]
    assert bers[0] > bers[1] > bers[2] and 0.1 < bers[0] < 0.4 and bers[2] < 0.02, bers
    # decisions on the same noisy IQ: GPU == oracle
    nf = 4
    data = payload(nf * g["bytes_per_frame"], seed=12)
    iq = torch.empty((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
    out = torch.empty((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
    std = bs.noise_std_for(CC, 10.0)
    m.tx(dev(data), nf, iq, noise_std=std, seed=1010)
    m.rx(iq, nf, bytes_out=out)
    h = host(iq)
    _, ob, _ = O.rx_batch(CC, h, nf, g["message_len"])
    assert np.array_equal(ob, host(out))
    clean = O.tx_batch(CC, data, nf)
    want = O.awgn(clean, std, seed=1010)
    assert rel_err(h - clean, want - clean) < 1e-6  # the channel model's tolerance on the noise


def test_full_size_config_b_every_frame_matches_oracle():
    """The bench workload (config 2: 8 192 config-B frames, Es/N0 10 dB) checked
    frame by frame: the GPU's clean tx IQ against the oracle's FFT path
    (1e-10 relative), and the GPU's rx of the noisy IQ against the oracle's
    rx of the same samples (every byte; constellation to 1e-9)."""
    m = modem("B")
    g = O.geometry(B)
    nf = 8192
    data = payload(nf * g["bytes_per_frame"], seed=77)
    d_data = dev(data)
    iq = torch.empty((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
    m.tx(d_data, nf, iq)
    want_iq = O.tx_batch(B, data, nf, threads=16)
    assert rel_err(host(iq), want_iq) < 1e-10
    del want_iq
    cons = torch.empty((nf * g["npts"],), dtype=torch.complex128, device="cuda")
    out = torch.empty((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
    m.tx(d_data, nf, iq, noise_std=float(np.sqrt(2.0 / 10.0)), seed=12)
    m.rx(iq, nf, constell_out=cons, bytes_out=out)
    h = host(iq)
    ocons, obytes, _ = O.rx_batch(B, h, nf, g["message_len"], threads=16)
    assert np.array_equal(host(out), obytes)
    assert rel_err(host(cons), ocons) < 1e-9


def _bit_errors(a: np.ndarray, b: np.ndarray) -> int:
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def test_config3_bench_workload_every_frame_matches_oracle():
    """bench.py's config-3 record at its size (BASELINE
    configs[2]): the 4 096 config-C frames per GPU (N = 4096, D = 2048, P = 64,
    cp = 1024, 16-QAM) of the job's counter-based payload, tx with fused AWGN at
    Es/N0 = 10 dB (seed 1010), then rx: every frame's bytes equal the oracle's
    rx of the same noisy samples, the constellation to 1e-9 (OFDM/modulation.cpp:
    53-87, Frame.cpp:73-96). Two BER-sweep points (4 and 16 dB, seed 1000 + SNR,
    the sweep's frame count): the GPU's bit-error counts equal the oracle's
    decisions on the same IQ, bit for bit.
    The channel is this repo's counter-based AWGN, not modem arithmetic: the
    GPU draws its Box-Muller on the FP32 transcendental units, so its noise
    agrees with the oracle's FP64 draw of the same counters to the channel
    model's tolerance, 1e-6 relative on the noise component (measured ~1e-7);
    the modem's own 1e-6 IQ bound applies to the noise-free tx (1e-10 here)."""
    from ofdm_synth import payload_bytes
    m = modem("C")
    g = O.geometry(CC)
    nf, msg, bpf = 4096, g["message_len"], g["bytes_per_frame"]
    es = 10.0 / 9.0  # mean energy of the reference's 16-QAM table (bench.py config3_leg)
    data = payload_bytes(0, nf * bpf)
    d = dev(data)
    iq = torch.empty((nf * msg,), dtype=torch.complex128, device="cuda")
    cons = torch.empty((nf * g["npts"],), dtype=torch.complex128, device="cuda")
    out = torch.empty_like(d)
    errs = torch.zeros((1,), dtype=torch.int64, device="cuda")
    std = float(np.sqrt(es / 10 ** (10.0 / 10)))
    m.tx(d, nf, iq, noise_std=std, seed=1010, sample_offset=0)
    m.rx(iq, nf, constell_out=cons, bytes_out=out, ref=d, bit_errors=errs)
    h = host(iq)
    ocons, obytes, _ = O.rx_batch(CC, h, nf, msg, threads=16)
    hb = host(out)
    assert np.array_equal(hb, obytes)  # every frame, every byte
    assert rel_err(host(cons), ocons) < 1e-9
    assert int(host(errs)[0]) == _bit_errors(obytes, data)
    del ocons, cons
    # the channel: noise component against the oracle's draw of the same counters
    f_chk = [0, 1, 2047, 4095]
    for f in f_chk:
        clean = O.tx_batch(CC, data[f * bpf:(f + 1) * bpf], 1)
        want = O.awgn(clean, std, seed=1010, sample_offset=f * msg)
        got = h[f * msg:(f + 1) * msg]
        assert rel_err(got - clean, want - clean) < 1e-6
    del h
    # two BER-sweep points: GPU bit-error counts == the oracle's on the same IQ
    nb = int(np.ceil(1e7 / (8 * bpf)))
    for db in (4, 16):
        errs.zero_()
        sd = float(np.sqrt(es / 10 ** (db / 10)))
        m.tx(d, nb, iq, noise_std=sd, seed=1000 + db, sample_offset=0)
        m.rx(iq, nb, bytes_out=out, ref=d, bit_errors=errs)
        hn = host(iq)[:nb * msg]
        _, ob, _ = O.rx_batch(CC, hn, nb, msg, threads=16)
        assert np.array_equal(host(out)[:nb * bpf], ob)
        assert int(host(errs)[0]) == _bit_errors(ob, data[:nb * bpf]) > 0
