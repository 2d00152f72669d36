"""tx on every instance of tx_kernel<LOGN, POINTS, NOISE, I16> the C ABI
reaches (35: tests/tx_cases.py names them and the 21 it cannot reach) and on
the branches the table of tests/tx_cases.py aims at: the fused AWGN in both
emit forms with cp in registers (cp = 0, T, N/4, 7T, N) and through the
general-cp path (cp = 1, odd, above T), past the 4096-workgroup grid with S
not dividing it, on every first-butterfly form, from a byte-wise payload for
each of its causes (an odd device pointer among them), at D > N/2 and D < T;
ofdm_fft_write at every LOGN on points off the constellation; ofdm_tx_frames
at LOGN 6, 9 and 12 and on 600 frames. tests/test_tx_cases.py asserts on the
CPU that the launches made here reach all of that, that the AWGN edge counters
are what they are listed as, and that assert_int16_match's band is all but
empty on every int16 output compared through it.

Per case one Modem, closed at the end of the test. Outputs at a frame stride of
message_len + 3 with a sentinel (9+9j, int16 77) between the frames.

Bars, the suite's own (test_gpu_parity.py, test_gpu_tx_sparse.py):
- noise-free samples within TOL = 1e-10 relative of O.tx_batch /
  O.frame_write / orc_fft_write (rel_err: the largest difference over the
  largest reference magnitude);
- int16 by assert_int16_match against the oracle's samples, and equal to
  trunc(mult x) of the launch's own f64 output;
- the noise component got - clean within TOL_NOISE = 1e-6 relative of
  O.awgn(clean) - clean, in each emit form separately (the forms may differ
  from each other by an FP32 ulp of the noise); the oracle applies the noise
  to the launch's nframes S L contiguous samples;
- the int16 output of a noisy launch equals the noise-free launch's: the wire
  samples carry no noise;
- a channel with noise_std 0, negative or NaN, the dead-group switch on
  against off, the call without an int16 output against the call with one, a
  graph replay against the eager launch: equal bit for bit.

Measured on the MI355X: the worst noise-free rel_err over all cases 8.1e-16
(N1024-D512-P16-cp256-k1-S3), the worst noise-component rel_err 1.5e-7 (the
same case; 1.2e-7 .. 1.5e-7 everywhere, at noise_std 1e-6 and 50 as at 0.3);
every equality held; under a second per test. At the AWGN edge counters, the
difference from the oracle's noise over the oracle's noise at that sample,
f64-only form / form with the int16 output: largest radius (u1 = 2^-24)
2.2e-8 / 6.4e-8; u2 = 0: 5.3e-8 / 3.6e-8; 1/4: 2.1e-8 / 7.8e-9; 1/2: 2.7e-8 /
3.0e-8; 3/4: 8.7e-8 / 4.7e-8, the same on a first CP sample, on a last body
sample and in symbol 4100 of 4200; radius 0 (u1 = 1): the noise-free launch's
sample bit for bit in both forms. These are records, not bars: the bar at
those samples is TOL_NOISE of the launch's largest noise sample.

What the module is expected to notice, one wrong line of tx_kernel each
(scratch builds, never committed):
- the noise counter one sample late (g0 + 1): every test_tx_modulate case and
  the graph test fail (so does test_gpu_tx_sparse.py at LOGN 9 and 11);
- awgn_sample_scaled without its scale: every case fails, in the <…, true,
  false> launches alone;
- the noise counted by memory position (frame * frame_stride + s L) instead
  of sym * L: every case fails here, and no other module notices (their noisy
  frames are contiguous);
- the header guarded by s == 1: the one-symbol frames of
  N4096-D2048-P64-cp1023-k4-S1 fail (with S > 1 symbol 1 writes the same
  header to the same place);
- the header written on the first trip of the grid only: the 600-frame
  test_tx_frames fails, and no other module notices;
- (f, s) of the next symbol from a division instead of the incremental
  bookkeeping: nothing fails, as it must.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import tx_cases as TC
from common import assert_int16_match, payload, rel_err
from test_gpu_tx_sparse import TOL, TOL_NOISE, both_ways

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

PAD = 64  # sentinel elements past every output


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the fixtures are read-only arrays


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def payload_at(data, alignment):
    """The payload on the device at `alignment` bytes past an allocation's start."""
    buf = torch.zeros((len(data) + alignment,), dtype=torch.uint8, device="cuda")
    view = buf[alignment:]
    view.copy_(torch.from_numpy(np.array(data)))
    assert view.data_ptr() % 4 == alignment % 4
    return view


def bits(a):
    """A host array's bit patterns (equality of these is bit-for-bit equality)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.kind in "cf" else a


def trunc16(x, mult):
    """FRAME_FORM::get_int16 on the host: trunc(mult x) per component, interleaved."""
    v = np.empty(x.shape + (2,))
    v[..., 0] = x.real * mult
    v[..., 1] = x.imag * mult
    return np.trunc(v).astype(np.int16).reshape(x.shape[:-1] + (2 * x.shape[-1],))


def modulate(m, d_data, nf, stride, i16, channel=None, noise_std=0.0, offset=0):
    """One ofdm_tx_modulate into sentinel-filled outputs: (iq,) or (iq, iq16).
    `channel`: an ofdm_channel passed through the C ABI as it is."""
    iq = torch.full((nf * stride,), TC.GAP_F64, dtype=torch.complex128, device="cuda")
    iq16 = torch.full((2 * nf * stride,), TC.GAP_I16, dtype=torch.int16, device="cuda") if i16 else None
    if channel is None:
        m.tx(d_data, nf, iq, frame_stride=stride, iq16_out=iq16, noise_std=noise_std, seed=TC.AWGN_SEED,
             sample_offset=offset)
    else:
        M.check(M.lib().ofdm_tx_modulate(m.h, d_data.data_ptr(), nf, iq.data_ptr(), stride,
                                         iq16.data_ptr() if i16 else None, C.byref(channel),
                                         torch.cuda.current_stream().cuda_stream))
    return (iq, iq16) if i16 else (iq,)


def split(outs, nf, stride, msg):
    """Host views (f64 (nf, msg), int16 (nf, 2 msg) or None) of one launch's
    outputs; the sentinels between the frames must have survived."""
    got = host(outs[0]).reshape(nf, stride)
    assert np.all(got[:, msg:] == TC.GAP_F64), "tx wrote between the frames (f64)"
    got16 = None
    if len(outs) == 2:
        got16 = host(outs[1]).reshape(nf, 2 * stride)
        assert np.all(got16[:, 2 * msg:] == TC.GAP_I16), "tx wrote between the frames (int16)"
        got16 = got16[:, :2 * msg]
    return got[:, :msg], got16


@pytest.mark.parametrize("name", TC.NAMES)
def test_tx_modulate(name):
    c = TC.CASES[name]
    g = O.geometry(c)
    nf, msg, L, S = TC.frames_of(name), g["message_len"], g["symbol_len"], c["num_symb"]
    x = TC.inputs(name, nf)
    stride, clean = x["stride"], x["clean"]
    assert stride == msg + 3
    m = M.Modem(c, 0)
    try:
        masks = TC.dead_masks(c)
        assert m.tx_sparse() == any(masks)  # the restated masks are the library's
        if masks:
            assert list(m.tx_dead_tables()[0]) == masks
        data = {}
        plain, wire = {}, {}  # per payload alignment: the noise-free launches' f64 / int16 outputs
        worst, worst_noise = 0.0, 0.0
        missed = []  # the launches over a bar: all of them are reported, not the first alone
        for _, rnf, entry, noise, i16, align, std, off in TC.runs(name):
            if entry != "tx":
                continue
            assert rnf == nf
            if align not in data:
                data[align] = payload_at(x["data"], align)
            d = data[align]
            outs = both_ways(m, lambda: modulate(m, d, nf, stride, i16, noise_std=std, offset=off))
            got, got16 = split(outs, nf, stride, msg)
            what = f"{name} <noise {noise}, i16 {i16}> align {align} std {std} offset {off}"
            if not noise:
                e = rel_err(got, clean)
                worst = max(worst, e)
                print(f"{what}: rel_err {e:.3e}")
                if not e < TOL:
                    missed.append(f"{what}: rel_err {e:.3e}")
                if align in plain:  # the f64-only instance and the one with the int16 output
                    assert torch.equal(plain[align], outs[0]), what
                plain[align] = outs[0]
                if i16:
                    assert_int16_match(got16, clean, c["mult"])
                    assert np.array_equal(got16, trunc16(got, c["mult"])), what
                    wire[align] = outs[1]
                if align:  # the byte-wise payload reads what the word-wise one does
                    assert torch.equal(outs[0], plain[0]), what
                # a channel that asks for no noise is no channel
                for bad in (0.0, -1.0, float("nan")):
                    ch = M.Channel(bad, TC.AWGN_SEED, TC.OFFSET0)
                    same = modulate(m, d, nf, stride, i16, channel=ch)
                    torch.cuda.synchronize()
                    assert all(torch.equal(a, b) for a, b in zip(outs, same)), f"{what}: noise_std {bad}"
                continue
            want = TC.noisy(name, nf, std, off)
            e = rel_err(got - clean, want - clean)
            worst_noise = max(worst_noise, e)
            print(f"{what}: noise rel_err {e:.3e}")
            if not e < TOL_NOISE:
                missed.append(f"{what}: noise rel_err {e:.3e}")
                continue
            if i16:
                assert torch.equal(outs[1], wire[align]), f"{what}: the wire samples carry noise"
            for _, _, kind, where, sym, j in TC.edge_at(name, off):
                f, at = sym // S, (sym % S) * L + j
                ref_noise = want[f, at] - clean[f, at]
                gpu_clean = complex(host(plain[0]).reshape(nf, stride)[f, at])
                d_noise = abs((got[f, at] - clean[f, at]) - ref_noise)
                biggest = np.abs(want - clean).max()
                if kind == "u1_one":  # radius 0: the clean sample, to one rounding of it
                    assert ref_noise == 0
                    dre, dim = abs(got[f, at].real - gpu_clean.real), abs(got[f, at].imag - gpu_clean.imag)
                    print(f"EDGE {name} i16={i16} {kind} {where} sym {sym}: |got - clean| = ({dre:.3e}, {dim:.3e})")
                    assert dre <= np.spacing(abs(gpu_clean.real)) and dim <= np.spacing(abs(gpu_clean.imag)), what
                else:
                    print(f"EDGE {name} i16={i16} {kind} {where} sym {sym}: |noise - oracle's| / |oracle's| = "
                          f"{d_noise / abs(ref_noise):.3e} (of the largest noise sample {d_noise / biggest:.3e})")
                assert d_noise < TOL_NOISE * biggest, what
        print(f"{name}: {TC.AIMS[name]}; worst rel_err {worst:.3e}, worst noise rel_err {worst_noise:.3e}")
        assert not missed, "\n".join(missed)
    finally:
        m.close()


@pytest.mark.parametrize("name", TC.NAMES)
def test_fft_write(name):
    c = TC.CASES[name]
    (nf,) = [r[1] for r in TC.runs(name) if r[2] == "fft_write"]
    n = nf * c["fft_size"] * c["num_symb"]
    pts = TC.points(name, nf)
    d_pts = dev(pts)
    m = M.Modem(c, 0)
    try:
        def run():
            fb = torch.full((n + PAD,), TC.GAP_F64, dtype=torch.complex128, device="cuda")
            m.fft_write(d_pts, nf, fb)
            return (fb,)

        (fb,) = both_ways(m, run)
        got = host(fb)
        assert np.all(got[n:] == TC.GAP_F64), "fft_write wrote past its output"
        e = rel_err(got[:n], TC.fft_write_ref(c, pts, nf).reshape(-1))
        print(f"{name} fft_write x{nf}: rel_err {e:.3e}")
        assert e < TOL
        assert np.array_equal(bits(host(d_pts)), bits(pts)), "the points were modified"
    finally:
        m.close()


FRAME_RUNS = sorted({(r[0], r[1]) for r in TC.runs() if r[2] == "tx_frames"})


@pytest.mark.parametrize("name,nf", FRAME_RUNS)
def test_tx_frames(name, nf):
    c = TC.CASES[name]
    g = O.geometry(c)
    flen, msg = g["frame_len"], g["message_len"]
    hlen = flen - msg
    forms = {r[4] for r in TC.runs(name) if r[2] == "tx_frames" and r[1] == nf}
    assert True in forms
    x = TC.inputs(name, nf)
    want = TC.frames_ref(name, nf)
    d = dev(x["data"])
    m = M.Modem(c, 0)
    try:
        def run(i16):
            fr = torch.full((nf * flen + PAD,), TC.GAP_F64, dtype=torch.complex128, device="cuda")
            fr16 = torch.full((2 * (nf * flen + PAD),), TC.GAP_I16, dtype=torch.int16, device="cuda") if i16 else None
            m.tx_frames(d, nf, fr, fr16)
            return (fr, fr16) if i16 else (fr,)

        fr, fr16 = both_ways(m, lambda: run(True))
        (only,) = both_ways(m, lambda: run(False))
        assert torch.equal(fr, only), "the call without frames16_out differs in f64"
        got, got16 = host(fr), host(fr16)
        assert np.all(got[nf * flen:] == TC.GAP_F64) and np.all(got16[2 * nf * flen:] == TC.GAP_I16)
        got, got16 = got[:nf * flen].reshape(nf, flen), got16[:2 * nf * flen].reshape(nf, 2 * flen)
        # every frame's [T2 | preamble] is frame 0's, bit for bit
        assert np.array_equal(bits(got[:, :hlen]), bits(np.tile(got[0, :hlen], (nf, 1))))
        assert np.array_equal(got16[:, :2 * hlen], np.tile(got16[0, :2 * hlen], (nf, 1)))
        e_h, e_m = rel_err(got[0, :hlen], want[0, :hlen]), rel_err(got[:, hlen:], want[:, hlen:])
        print(f"{name} tx_frames x{nf}: header rel_err {e_h:.3e}, message rel_err {e_m:.3e}")
        assert e_h < TOL and e_m < TOL
        assert np.array_equal(got16, trunc16(got, c["mult"])), "int16 is not trunc(mult x) of the f64 output"
        if TC.int16_by_oracle((name, nf, "tx_frames", False, True)):
            assert_int16_match(got16[:, :2 * hlen], want[:, :hlen], c["mult"])
            assert_int16_match(got16, want, c["mult"])
        # the message part is ofdm_tx_modulate's
        iq, iq16 = modulate(m, d, nf, x["stride"], True)
        tx, tx16 = split((iq, iq16), nf, x["stride"], msg)
        assert np.array_equal(bits(got[:, hlen:]), bits(tx))
        assert np.array_equal(got16[:, 2 * hlen:], tx16)
    finally:
        m.close()


def test_noisy_launch_replays_from_a_graph():
    """One ofdm_tx_modulate with fused AWGN and the int16 output, general cp,
    4200 symbols on 4096 workgroups, captured and replayed (test_gpu_graph's
    protocol, default queue settings): equal to the eager launch bit for bit,
    on the capture's payload and on another written in place."""
    from test_gpu_graph import load, out_buf, replay_protocol
    name = TC.GRID_CASE
    c = TC.CASES[name]
    g = O.geometry(c)
    nf, msg = TC.MANY, g["message_len"]
    assert nf * c["num_symb"] > TC.TX_MAX_GRID and c["cp_size"] % (c["fft_size"] // 8)
    cases = [TC.inputs(name, nf)["data"], payload(nf * g["bytes_per_frame"], TC.case_seed(name) + 5000)]
    d = dev(cases[0])
    m = M.Modem(c, 0)
    try:
        live = {"iq": nf * msg, "iq16": 2 * nf * msg}
        outs = {"iq": out_buf(live["iq"], torch.complex128), "iq16": out_buf(live["iq16"], torch.int16)}
        _, _, r1, r2, _ = replay_protocol(
            lambda: m.tx(d, nf, outs["iq"], iq16_out=outs["iq16"], noise_std=TC.NOISE_STD, seed=TC.AWGN_SEED,
                         sample_offset=TC.OFFSET0),
            lambda i: load(d, cases[i]), outs, live)
        clean = TC.inputs(name, nf)["clean"].reshape(-1)
        want = TC.noisy(name, nf, TC.NOISE_STD, TC.OFFSET0).reshape(-1)
        assert rel_err(r1["iq"][:nf * msg] - clean, want - clean) < TOL_NOISE
        assert_int16_match(r1["iq16"][:2 * nf * msg], clean, c["mult"])
        clean2 = O.tx_batch(c, cases[1], nf, threads=8)
        assert rel_err(r2["iq"][:nf * msg] - clean2, want - clean) < TOL_NOISE  # the same noise on the new samples
    finally:
        m.close()
