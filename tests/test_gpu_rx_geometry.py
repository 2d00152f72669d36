"""The batched rx on every non-stream kernel instance and on geometries off
the D = N/2 diagonal: rx_kernel and rx_soft_kernel at LOGN 6..12 x STAGED x
I16, rx_wide_kernel<9..12>, and the branches of ofdm_rx_body.inc that the
table of tests/rx_geometry_cases.py aims at (per-symbol packing, the channel
read from memory, byte-wise packing, masked lanes at every T, odd cp, cp = 1,
cp = N, P = 2, P near T). tests/test_rx_geometry_cases.py asserts on the CPU
that the launches made here reach all of them and that the inputs are well
conditioned; here the same dispatch rule is asserted with the device's own
compute-unit count. The stream-mode (SYNC) instances are the stream tests'.

Per case, one Modem: inputs from the oracle (O.tx_batch + O.awgn at Es/N0 =
12 dB) at a frame stride of message_len + 3 with NaN (int16: -32768) between
the frames; 3 frames, and from N = 512 on also CUs/2 + 2 frames (the
persistent kernel where 3 frames take the few-frame one).

Bars, all the suite's own: points within 1e-10 relative of the oracle's
(test_gpu_parity.py), bytes and bit-error counts equal to the oracle's, the
divided points within 1e-14 of read_out / chan, LLRs at test_gpu_soft.py's
bars, tx within 1e-10 and its int16 by assert_int16_match; everything said to
be equal between two launches is equal bit for bit.

Measured on the MI355X (256 compute units, so 3 and 130 frames): the worst
rx rel_err over all cases 7.8e-15 (N1024-D504-P126-cp255-k2-S9), the worst tx
rel_err 9.9e-16; every byte, count and bit-for-bit equality held; 2.0 - 2.7 s
per case, process start included.

What the module is expected to notice, one wrong kernel each (a scratch build
of ofdm_rx_body.inc with all three, never committed; the suite's other rx
modules, 195 tests of test_gpu_parity / rx_emit / soft / decision_boundary /
entry_gaps, passed on it):
- the per-symbol pack reading its decisions one carrier late
  (pack(s * bps, (s + 1) * bps, 1)): N64-D32-P8-cp3-k6-S40 and
  N512-D248-P62-cp127-k1-S35 fail (bytes), the only cases with S*D > 16 N;
- the channel divisor read from memory at carrier d ^ 1: N128-D64-P4-cp16-k2-S17
  fails (divided points), and so would the two cases above;
- by_word no longer asking for bytes_per_frame % 4 == 0: N64-D8-P2-cp64-k1-S7
  (7 bytes per frame) fails at 3 frames, N512-D72-P6-cp5-k2-S7 (126) and
  N4096-D2040-P204-cp1023-k2-S1 (510) at 130 frames only: at 3 frames they
  take rx_wide_kernel, which has its own packing code."""
import numpy as np
import pytest

import oracle as O
import rx_geometry_cases as RG
from common import assert_int16_match, rel_err
from test_gpu_parity import TOL
from test_gpu_soft import FMTS, check_against_oracle, llr_buffer, take_llr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

PAD = 64  # sentinel elements past every output
BYTE_SENTINEL = 0xA5
ERR_START = 1000  # the error counter is added to, not set


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the fixtures are read-only arrays


def bits_of(a):
    """A host array as integers: equality bit for bit (NaN included)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.kind in "cf" and a.dtype.itemsize in (8, 16) else a


class Outputs:
    """One launch's outputs, each followed by PAD sentinel elements."""

    def __init__(self, c, nf, points=True, read=False, errors=True):
        g = O.geometry(c)
        self.npts, self.nbytes = nf * g["npts"], nf * g["bytes_per_frame"]

        def points_buf():
            return torch.full((self.npts + PAD,), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")

        self.cons = points_buf() if points else None
        self.read = points_buf() if read else None
        self.out = torch.full((self.nbytes + PAD,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
        self.errs = torch.full((1 + PAD,), ERR_START, dtype=torch.int64, device="cuda") if errors else None

    def host(self):
        """dict(cons, read, bytes, errs) on the host; the sentinels must have survived."""
        torch.cuda.synchronize()
        r = {}
        for key, buf, n in (("cons", self.cons, self.npts), ("read", self.read, self.npts)):
            if buf is not None:
                h = buf.cpu().numpy()
                assert np.isnan(h[n:].real).all() and np.isnan(h[n:].imag).all(), f"wrote past {key}"
                assert not np.isnan(h[:n]).any(), f"{key}: a point was not written"
                r[key] = h[:n]
        h = self.out.cpu().numpy()
        assert np.all(h[self.nbytes:] == BYTE_SENTINEL), "wrote past the bytes"
        r["bytes"] = h[:self.nbytes]
        if self.errs is not None:
            h = self.errs.cpu().numpy()
            assert np.all(h[1:] == ERR_START), "wrote past the error counter"
            r["errs"] = int(h[0]) - ERR_START
        return r


def assert_same(a, b, what, keys=("cons", "bytes", "errs")):
    for key in keys:
        if key == "errs":
            assert a[key] == b[key], f"{what}: bit errors {a[key]} != {b[key]}"
        else:
            assert np.array_equal(bits_of(a[key]), bits_of(b[key])), f"{what}: {key} differ"


def soft_launch(m, c, x, nf, stride, fmt, scale, fs, ref, i16):
    """One ofdm_rx_demod_soft launch with every output; the shapes check_against_oracle takes."""
    g = O.geometry(c)
    k = c["mod_type"]
    o = Outputs(c, nf)
    llr = llr_buffer(nf * g["npts"] * k, fmt)
    m.rx_soft(x, nf, llr, scale, FMTS[fmt][0], frame_scale=fs, frame_stride=stride, constell_out=o.cons[:o.npts],
              bytes_out=o.out, ref=ref, bit_errors=o.errs, i16=i16)
    r = o.host()
    r["llr"] = take_llr(llr, nf * g["npts"] * k).reshape(nf, g["npts"], k)
    return r


@pytest.mark.parametrize("name", RG.NAMES)
def test_rx_geometry(name):
    c = RG.CASES[name]
    g = O.geometry(c)
    k, D, bpf, npf = c["mod_type"], c["num_data_subc"], g["bytes_per_frame"], g["npts"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    counts = RG.frame_counts(c, cus)
    nmax = max(counts)

    # the launches below take the instances the case is in the table for
    for entry, nf, i16, soft, with_chan in RG.runs(name, cus):
        assert RG.expected_instance(c, nf, i16, soft, cus) == RG.meant_instance(name, nf, i16, soft), (
            f"{entry} x{nf} does not take the instance it is meant for on {cus} compute units")

    x = RG.inputs(name, nmax)
    assert x["edge"] >= RG.EDGE_BAR  # (the CPU test's, on this device's frame count)
    stride = x["stride"]
    assert stride == g["message_len"] + 3 and np.isnan(x["iq"][stride - 1])
    m = M.Modem(c, 0)
    d_iq, d_ref = dev(x["iq"]), dev(x["ref"])
    d_chan = dev(RG.channel(name, nmax))
    worst = 0.0
    hard = {}
    for nf in counts:
        # ---- f64 rx: points, bytes, bit errors
        o = Outputs(c, nf)
        m.rx(d_iq, nf, frame_stride=stride, constell_out=o.cons[:o.npts], bytes_out=o.out, ref=d_ref,
             bit_errors=o.errs)
        r = hard[nf] = o.host()
        want_c, want_b = x["cons"][:nf * npf], x["bytes"][:nf * bpf]
        e = rel_err(r["cons"], want_c)
        worst = max(worst, e)
        assert e < TOL, f"x{nf}: points {e:.2e} from the oracle's"
        assert np.array_equal(r["bytes"], want_b), f"x{nf}: bytes differ from the oracle's"
        assert r["errs"] == RG.bit_errors(want_b, x["ref"][:nf * bpf]) > 0
        # ---- bytes only: a staged geometry stages in the context's own scratch
        o = Outputs(c, nf, points=False, errors=False)
        m.rx(d_iq, nf, frame_stride=stride, bytes_out=o.out)
        assert np.array_equal(o.host()["bytes"], r["bytes"]), f"x{nf}: bytes-only launch"
        # ---- with a channel divisor: read_out is the rx without it, the points are read_out / chan
        o = Outputs(c, nf, read=True, errors=False)
        m.rx_read(d_iq, nf, d_chan, o.read[:o.npts], frame_stride=stride, chan_stride=D, constell_out=o.cons[:o.npts],
                  bytes_out=o.out)
        rc = o.host()
        assert np.array_equal(bits_of(rc["read"]), bits_of(r["cons"])), f"x{nf}: read_out is not the plain rx"
        ch = np.tile(RG.channel(name, nf).reshape(nf, 1, D), (1, c["num_symb"], 1)).reshape(-1)
        assert rel_err(rc["cons"], rc["read"] / ch) < 1e-14, f"x{nf}: divided points"
        assert np.array_equal(rc["bytes"], O.demod(k, rc["cons"])[0]), f"x{nf}: bytes are not the points' decisions"
        # the same through ofdm_rx_demod with the divisor and a reference
        o = Outputs(c, nf)
        m.rx(d_iq, nf, frame_stride=stride, chan=d_chan, chan_stride=D, constell_out=o.cons[:o.npts],
             bytes_out=o.out, ref=d_ref, bit_errors=o.errs)
        rd = o.host()
        assert_same(rd, rc, f"x{nf}: rx with a divisor against rx_read", keys=("cons", "bytes"))
        assert rd["errs"] == RG.bit_errors(rc["bytes"], x["ref"][:nf * bpf])
    if len(counts) == 2:  # the persistent launch's first frames are the few-frame launch's
        few, big = hard[counts[0]], hard[counts[1]]
        n = counts[0]
        assert np.array_equal(bits_of(big["cons"][:n * npf]), bits_of(few["cons"]))
        assert np.array_equal(big["bytes"][:n * bpf], few["bytes"])
    assert np.array_equal(bits_of(d_iq.cpu().numpy()), bits_of(x["iq"])), "the input was modified"

    # ---- int16 rx equals rx on the same integers as doubles, and the oracle on those
    nf = RG.FEW
    w = RG.i16_input(name)
    assert w["edge"] >= RG.EDGE_BAR
    d_x16, d_w = dev(w["x16"]), dev(w["iq"])
    ref3 = x["ref"][:nf * bpf]
    o16, o64 = Outputs(c, nf), Outputs(c, nf)
    m.rx_i16(d_x16, nf, frame_stride=stride, constell_out=o16.cons[:o16.npts], bytes_out=o16.out, ref=d_ref,
             bit_errors=o16.errs)
    m.rx(d_w, nf, frame_stride=stride, constell_out=o64.cons[:o64.npts], bytes_out=o64.out, ref=d_ref,
         bit_errors=o64.errs)
    r16, r64 = o16.host(), o64.host()
    assert_same(r16, r64, "rx_i16 against rx on the converted samples")
    e = rel_err(r16["cons"], w["cons"])
    worst = max(worst, e)
    assert e < TOL, f"int16: points {e:.2e} from the oracle's"
    assert np.array_equal(r16["bytes"], w["bytes"]) and r16["errs"] == RG.bit_errors(w["bytes"], ref3) > 0
    assert np.array_equal(d_x16.cpu().numpy(), w["x16"]), "the int16 input was modified"

    # ---- soft rx, both formats on both inputs: the hard rx's outputs and the model's LLRs
    scale = 4.0
    fs = np.random.default_rng(RG.case_seed(name)).uniform(0.25, 4.0, nf)
    d_fs = dev(fs)
    for inp, d_x, hard_r, E in (("f64", d_iq, hard[nf], x["cons"][:nf * npf]), ("i16", d_x16, r16, w["cons"])):
        soft = {fmt: soft_launch(m, c, d_x, nf, stride, fmt, scale, d_fs, d_ref, inp == "i16") for fmt in FMTS}
        for fmt, r in soft.items():
            assert_same(r, hard_r, f"soft {inp} {fmt} against the hard rx")
            r["cons"] = r["cons"].reshape(nf, -1)
        check_against_oracle(c, E.reshape(nf, -1), soft["f32"], soft["i8"], scale, fs, f"{name} {inp}")

    # ---- tx at the same geometry
    d_data = dev(x["data"][:nf * bpf])
    L = g["message_len"]
    iq = torch.full((nf * stride,), complex(9.0, 9.0), dtype=torch.complex128, device="cuda")
    iq16 = torch.full((nf * stride * 2,), 77, dtype=torch.int16, device="cuda")
    m.tx(d_data, nf, iq, frame_stride=stride, iq16_out=iq16)
    torch.cuda.synchronize()
    got = iq.cpu().numpy().reshape(nf, stride)
    got16 = iq16.cpu().numpy().reshape(nf, stride * 2)
    want = x["clean"][:nf * stride].reshape(nf, stride)
    e_tx = rel_err(got[:, :L], want[:, :L])
    assert e_tx < TOL, f"tx {e_tx:.2e} from the oracle's"
    assert np.all(got[:, L:] == complex(9.0, 9.0)) and np.all(got16[:, 2 * L:] == 77), "tx wrote between the frames"
    assert_int16_match(got16[:, :2 * L], want[:, :L], c["mult"])
    m.close()
    print(f"{name}: {RG.AIMS[name]}; frames {counts}; worst rx rel_err {worst:.3e}, tx rel_err {e_tx:.3e}")
