"""The life cycle of a context: on a fresh ofdm_ctx every member that is
created or grown on demand is made to exist (the staged rx scratch and the CFO
scratch, each grown once; a second CFO plan; the stream receiver's scratch,
pinned staging, events and side stream; the phase-timing events), the context
is destroyed, a new one is created and the same calls repeated: every output
of the second life equals the first bit for bit.

Two geometries, each with num_symb = 9 (the staged rx and its scratch): the
default, and the smallest supported one (N = 64, D = 32, P = 4, cp = 16, T2 size
64, pr_sin_len 32). The small one takes num_pr_symb = 4: with one preamble
symbol its pilot_freq_sinh form is 80 = 5 * 16 samples, which no kernel covers
(tests/test_gpu_channel.py asserts that refusal), and sync_frames and the
stream decode need that form.

No free-memory figure is read (it is device-wide), and nothing is made to fail.
"""
import numpy as np
import pytest

import oracle as O
from common import cfg, payload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

# (config, nsym of the second CFO form: 1280 = 5 * 256 and 640 = 5 * 128 samples)
CASES = {
    "D_s9": (cfg(O.DEFAULT, num_symb=9), 2),
    "N64_s9": (cfg(O.DEFAULT, fft_size=64, num_data_subc=32, num_pilot_subc=4, cp_size=16, t2sin_size=64,
                   pr_sin_len=32, num_symb=9, num_pr_symb=4), 8),
}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def one_life(c, nsym2, data, x5):
    """Every call of the list on a new context; returns the outputs by name."""
    g = O.geometry(c)
    flen, t2, bpf = g["frame_len"], c["t2sin_size"], g["bytes_per_frame"]
    body = t2 + g["preamble_len"]
    out = {}
    m = M.Modem(c, 0)
    try:
        # 3 full frames, one frame of silence behind them (the stream call's input)
        fr = torch.zeros((4 * flen,), dtype=torch.complex128, device="cuda")
        m.tx_frames(dev(data[: 3 * bpf]), 3, fr)
        out["tx_frames"] = host(fr)
        # rx without a constellation output: 2 frames, then 5 (the scratch grows)
        dx = dev(x5)
        for nf in (2, 5):
            b = torch.zeros((nf * bpf,), dtype=torch.uint8, device="cuda")
            m.rx(dx[body:], nf, frame_stride=flen, bytes_out=b)
            out[f"rx_{nf}"] = host(b)
            assert np.array_equal(out[f"rx_{nf}"], data[: nf * bpf])
        # sync_frames keeping no CFO: 2 frames, then 5 (the CFO scratch grows)
        for nf in (2, 5):
            s = dx.clone()
            m.sync_frames(s[t2:], nf, flen, cfo_out=None)
            out[f"sync_{nf}"] = host(s)
        # a CFO estimate at a second form length: a second plan
        est = torch.zeros((3,), dtype=torch.float64, device="cuda")
        m.cfo_estimate(dx[t2:], 3, flen, nsym2, est)
        out["cfo"] = host(est)
        # one stream call on the 3 frames, with the phase events
        m.stream_timing(True)
        mf = 8
        pbs = torch.full((mf,), -1, dtype=torch.int64, device="cuda")
        sb = torch.zeros((mf * bpf,), dtype=torch.uint8, device="cuda")
        sc = torch.zeros((mf * g["npts"],), dtype=torch.complex128, device="cuda")
        scfo = torch.zeros((mf,), dtype=torch.float64, device="cuda")
        found = m.rx_stream(fr, 4 * flen, mf, pb_out=pbs, bytes_out=sb, constell_out=sc, cfo_out=scfo)
        assert 1 <= found <= 3
        out["stream_nframes"] = np.array([found])
        out["stream_pb"], out["stream_bytes"] = host(pbs), host(sb)
        out["stream_constell"], out["stream_cfo"] = host(sc), host(scfo)
    finally:
        torch.cuda.synchronize()
        m.close()
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_second_life_equals_the_first(name):
    c, nsym2 = CASES[name]
    g = O.geometry(c)
    bpf = g["bytes_per_frame"]
    data = payload(5 * bpf, seed=11)
    x5 = np.concatenate([O.frame_write(c, data[f * bpf:(f + 1) * bpf]) for f in range(5)])
    first = one_life(c, nsym2, data, x5)
    second = one_life(c, nsym2, data, x5)
    assert sorted(first) == sorted(second)
    for key in first:
        assert first[key].tobytes() == second[key].tobytes(), key
