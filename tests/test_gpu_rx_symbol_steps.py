"""rx_kernel's symbol steps as straight-line code (ofdm_rx_body.inc): with the
register window, step s is compiled with s and its window row as constants
and the steps are left at the first s >= S; the next symbol's prefetch is
issued after the transform's first pass. What is new is the early exit, the
per-symbol register sets and their carrying over the frame loop, so:

- every S from 1 to 8 at N = 64 (T = 8, less than a wave), at N = 512 with D
  off the 64-carrier grid (the emit through LDS) and at N = 2048 with D = 1024
  (QPSK: the fast emit); k = 2 and k = 4, from f64 and from int16 input, on
  enough frames that the persistent kernel runs and not the few-frame one;
- at N = 64, three times as many frames as resident workgroups and five more:
  every workgroup takes a second and a third frame (symbol 0 by DMA during
  the previous frame's epilogue);
- a cp that is no multiple of T;
- rx_soft_kernel, the staged kernels (S = 9, the rolled step) and the stream
  decode's SYNC instances (the phase ramp ahead of the first pass), S = 8 and
  S = 5.

Bars: bytes and bit-error counts equal to the oracle's, points within 1e-9
relative of the oracle's; LLRs at test_gpu_soft.py's bars; the stream's frames
at test_gpu_stream.py's.

Measured on the MI355X (256 compute units: 138 and 6 149 frames): the worst
rel_err of any case 2.1e-15; every byte and count held; the module's 32 tests
take 4.5 s."""
import numpy as np
import pytest

import oracle as O
import rx_geometry_cases as RG
from common import B, cfg, impaired_stream, payload, rel_err
from test_gpu_rx_geometry import Outputs, assert_same, soft_launch
from test_gpu_soft import FMTS, check_against_oracle
from test_gpu_stream import check_against_oracle as check_stream
from test_gpu_stream import run_stream

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

TOL = 1e-9
SNR_DB = 12.0
RX_WAVES_PER_CU = 8  # rx_launch_n's persistent grid: resident waves per CU


def geom(N, D, P, cp, **kw):
    c = dict(fft_size=N, num_data_subc=D, num_pilot_subc=P, cp_size=cp, **kw)
    if N + cp < O.DEFAULT["pr_sin_len"]:  # the context's preamble template must fit the preamble
        c["pr_sin_len"] = 64
    return cfg(O.DEFAULT, **c)


GEOMS = {
    "N64": geom(64, 24, 4, 16),
    "N512": geom(512, 200, 8, 128),
    "N2048": geom(2048, 1024, 32, 512),
}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frames(c, nf, seed):
    """nf noisy frames of config c from the oracle, as f64 and in the wire
    format, with the oracle's rx of each: dict(ref, iq, cons, bytes, errs,
    x16, cons16, bytes16, errs16)."""
    g = O.geometry(c)
    bpf, msg = g["bytes_per_frame"], g["message_len"]
    data, ref = payload(nf * bpf, seed), payload(nf * bpf, seed + 1)  # ref is not the payload: errors to count
    es = float(np.mean(np.abs(O.constellation(c["mod_type"])) ** 2))
    iq = O.awgn(O.tx_batch(c, data, nf, threads=8), np.sqrt(es / 10 ** (SNR_DB / 10)), seed=seed + 2, threads=8)
    cons, obytes, errs = O.rx_batch(c, iq, nf, msg, ref=ref, threads=8)
    x16 = np.ascontiguousarray(O.get_int16(iq, c["mult"]).reshape(-1))
    w = x16.astype(np.float64)
    cons16, bytes16, errs16 = O.rx_batch(c, w[0::2] + 1j * w[1::2], nf, msg, ref=ref, threads=8)
    return dict(ref=ref, iq=iq, cons=cons, bytes=obytes, errs=errs, x16=x16, cons16=cons16, bytes16=bytes16,
                errs16=errs16)


def check_rx(m, c, nf, x, what):
    """m.rx and m.rx_i16 on x against the oracle; returns the f64 launch's outputs."""
    d_ref = dev(x["ref"])
    res = None
    for inp in ("f64", "i16"):
        o = Outputs(c, nf)
        if inp == "f64":
            m.rx(dev(x["iq"]), nf, constell_out=o.cons[:o.npts], bytes_out=o.out, ref=d_ref, bit_errors=o.errs)
            want_c, want_b, want_e = x["cons"], x["bytes"], x["errs"]
        else:
            m.rx_i16(dev(x["x16"]), nf, constell_out=o.cons[:o.npts], bytes_out=o.out, ref=d_ref, bit_errors=o.errs)
            want_c, want_b, want_e = x["cons16"], x["bytes16"], x["errs16"]
        r = o.host()
        e = rel_err(r["cons"], want_c)
        print(f"{what} {inp} x{nf}: points {e:.3e} from the oracle's")
        assert e < TOL, f"{what} {inp}: points {e:.2e} from the oracle's"
        assert np.array_equal(r["bytes"], want_b), f"{what} {inp}: bytes differ from the oracle's"
        assert r["errs"] == want_e > 0, f"{what} {inp}: bit errors"
        res = res or r
    return res


def persistent_frames(c, S):
    """More frames than the few-frame kernel takes (CUs / 2), a count that varies with S."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nf = cus // 2 + 2 + S
    for i16 in (False, True):
        assert RG.expected_instance(c, nf, i16, False, cus) == ("rx_kernel", c["fft_size"].bit_length() - 1, False, i16)
    return nf


@pytest.mark.parametrize("S", range(1, 9))
@pytest.mark.parametrize("name", list(GEOMS))
def test_every_symbol_count(name, S):
    for k in (2, 4):
        c = cfg(GEOMS[name], num_symb=S, mod_type=k)
        assert RG.valid(c)
        nf = persistent_frames(c, S)
        m = M.Modem(c, 0)
        # the context offers the fast emit at QPSK; the kernel takes it at
        # N = 2048 (D a multiple of 64), the other geometries emit through LDS
        assert m.rx_emit_fast() == (k == 2)
        check_rx(m, c, nf, frames(c, nf, seed=100 * S + k), f"{name}-S{S}-k{k}")
        m.close()


@pytest.mark.parametrize("S", [5, 8])
def test_several_frames_per_workgroup(S):
    c = cfg(GEOMS["N64"], num_symb=S, mod_type=2)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nf = 3 * RX_WAVES_PER_CU * cus + 5  # T = 8: one wave per workgroup
    m = M.Modem(c, 0)
    x = frames(c, nf, seed=7 + S)
    big = check_rx(m, c, nf, x, f"N64-S{S}-persistent")
    # the first frames of the long launch are a short launch's, bit for bit
    few = 3
    g = O.geometry(c)
    o = Outputs(c, few, errors=False)
    m.rx(dev(x["iq"][:few * g["message_len"]]), few, constell_out=o.cons[:o.npts], bytes_out=o.out)
    r = o.host()
    assert np.array_equal(r["cons"].view(np.uint64), big["cons"][:few * g["npts"]].view(np.uint64))
    assert np.array_equal(r["bytes"], big["bytes"][:few * g["bytes_per_frame"]])
    m.close()


def test_cp_no_multiple_of_T():
    c = cfg(geom(512, 200, 8, 37), num_symb=6, mod_type=2)  # T = 64
    assert RG.valid(c) and c["cp_size"] % (c["fft_size"] // 8)
    nf = persistent_frames(c, 6)
    m = M.Modem(c, 0)
    check_rx(m, c, nf, frames(c, nf, seed=37), "N512-cp37-S6")
    m.close()


def test_staged_keeps_the_rolled_step():
    c = cfg(GEOMS["N512"], num_symb=9, mod_type=2)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nf = 5
    for i16 in (False, True):
        assert RG.expected_instance(c, nf, i16, False, cus) == ("rx_kernel", 9, True, i16)
    m = M.Modem(c, 0)
    check_rx(m, c, nf, frames(c, nf, seed=9), "N512-S9-staged")
    m.close()


@pytest.mark.parametrize("S", [3, 8])
def test_soft_kernel(S):
    c = cfg(GEOMS["N512"], num_symb=S, mod_type=4)
    nf = 4
    m = M.Modem(c, 0)
    x = frames(c, nf, seed=50 + S)
    hard = check_rx(m, c, nf, x, f"N512-S{S}-hard")
    scale = 4.0
    fs = np.random.default_rng(S).uniform(0.25, 4.0, nf)
    soft = {fmt: soft_launch(m, c, dev(x["iq"]), nf, O.geometry(c)["message_len"], fmt, scale, dev(fs), dev(x["ref"]),
                             False) for fmt in FMTS}
    for fmt, r in soft.items():
        assert_same(r, hard, f"soft {fmt} against the hard rx")
        r["cons"] = r["cons"].reshape(nf, -1)
    check_against_oracle(c, x["cons"].reshape(nf, -1), soft["f32"], soft["i8"], scale, fs, f"N512-S{S}")
    m.close()


@pytest.mark.parametrize("name,c", [("B", B), ("B_s5_qam16", dict(B, num_symb=5, mod_type=4))])
def test_stream_decode_through_the_body(name, c):
    # staged_decode = 1: the located frames take the cfo -> params -> rx
    # kernels, rx_kernel<11, false, false, SYNC> among them
    x, _ = impaired_stream(c, 6, seed=31)
    want = check_stream(c, x, run_stream(c, x, chunk=40000, tuning=dict(staged_decode=1)))
    assert len(want) >= 3
