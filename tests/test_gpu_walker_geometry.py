"""The stream receiver on every walker instance and on the decode kernels no
other stream test launches (fixtures: tests/walker_cases.py, checked on the
CPU in tests/test_walker_cases.py).

Walker cases: stream_walk_kernel<6..11> in both stream formats, the FP32 T2
screen at G = 16, 8, 4 and 2, the FP64-only scan with two and four waves per
transform, the FFT preamble search in 1 to 72 windows (last windows of 1 to 384
lags) and the direct certified search at T2sin_size 64 to 1024. Per case, one
Modem and: the config's ring (three frames), the continuous walk and a ring of
two frames; chunks of 1.3 and of 5 frames, the small one also host-stitched
(lookback = 0); exact_search = 1, pre_f32 = 0 and t2_f32 = 0 at the small
chunk; the int16 form of the stream against the f64 call on the converted
samples; the T2 size's wire capture (exact-zero silences) in both formats,
ring and continuous. Decode cases: the narrow fused kernel at S = 1..8, P =
2..64, D = 8..248 and every modulation, with the staged kernels on the same
list (stream_params_kernel<9>, rx_stream2), and the staged stream kernels at
N = 64, 128, 256 and 4096 (cfo_kernel<6,1>, <7,1>, <8,1>, <6,5>, <12,1> with
`starts`), f64 and int16.

Bars, all tests/test_gpu_stream.py's check_against_oracle: the pb list and the
frame count of the oracle's ring walk, CFO equal, constellation within 1e-9
relative, every byte equal. Everything said to be equal between two GPU runs
is equal bit for bit. Every output buffer carries sentinels past the frames
found (run_guarded).

The stream call refuses a walker whose LDS passes 160 KB before anything is
issued (OFDM_ERR_UNSUPPORTED): T2sin_size = 2048 with pr_sin_len 450 and 640,
and T2sin_size = 4096, which has no walker. T2sin_size = 2048 has no direct
search at all: the direct form of WalkLds<11> fits up to pr_sin_len = 413,
where the FFT search is used, so the largest accepted length is 449 (the
T2048-L449 case).

The search's last lag (test_preamble_search_ends_at_its_last_lag): per walker
case a frame whose first passing lag lies in the search's last lags (lag C - 1
itself where the FFT search's last window holds one lag) and one whose first
passing lag is C or just past it; the first is located, the second is not.

Measured on the MI355X (256 compute units): the 43 tests take 5.4 s, process
start included; a walker case 0.04 - 0.21 s (the first one 0.58 s with the
device's start), an edge case up to 0.12 s, a decode case 0.01 - 0.06 s. The
worst constellation rel_err: walker table 5.4e-14 (T128-L128), decode table
4.0e-13 (N4096-cp0; narrow fused 2.3e-13, fused-S1-P64). Every list, CFO,
byte and bit-for-bit equality held.

What the module is expected to notice, one wrong value each in
stream_walk_kernel (three scratch builds of csrc/ofdm_sync.hip, never
committed; each was also run against the rest of the suite, 1512 tests):
- the FP32 screen posting its B-block hit as g instead of g + G: the ten
  walker cases with a screen (T2sin_size 64 .. 512) and seven decode cases
  fail here; the rest of the suite notices it too (222 failures in the
  stream modules, whose walks are at T2sin_size 256 and 512);
- t2_eval64 summing its first wave's partial sums only (red[g * NW] for every
  w): T1024-L128, T1024-L449, T1024-L640, T2048-L64 and T2048-L449 fail, the
  five cases with more than one wave per transform; the rest of the suite
  passes;
- the FFT search's last window taken whole (nl = Q): the eight edge cases
  whose FFT search has a partial last window and a message no shorter than
  the marker fail (T64-L64, T64-L449, T128-L128, T256-L300, T256-L449,
  T512-L64, T1024-L128, T1024-L449), on the frame past lag C - 1 that must not
  be located; the impaired streams and captures alone do not notice it (their
  first passing lag is never among the last), nor does the rest of the suite.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import walker_cases as W
from common import D, impaired_stream, rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402
from test_gpu_stream import check_against_oracle, dev, host, modem  # noqa: E402
from test_gpu_stream_backends import MF, Outputs, call, run_guarded, same_bits  # noqa: E402

ERR_UNSUPPORTED = -2
PARTS = ("frames", "pb", "bytes", "constellation", "cfo")


def assert_same(got, ref, what):
    """Two GPU runs, bit for bit: frame count, pb list, bytes, constellation, CFO."""
    assert got[0] == ref[0], f"{what}: {got[0]} frames, {ref[0]} in the other run"
    for part, a, b in zip(PARTS[1:], got[1:], ref[1:]):
        assert same_bits(a, b), f"{what}: {part} differs"


def worst_rel_err(c, x, got):
    """The largest constellation rel_err of a run that passed check_against_oracle (for the record)."""
    g = O.geometry(c)
    span = g["preamble_len"] + g["message_len"]
    return max([rel_err(got[3][f], O.decode_frame(c, W.frame_at(x, int(pb), span))[1])
                for f, pb in enumerate(got[1])], default=0.0)


def assert_input_untouched(m, c, x, i16, ref, chunk):
    """One more call on a device buffer that is compared with the host's afterwards."""
    dx = dev(x)
    o = Outputs(c, MF)
    nf = call(m, o, dx, len(x) // 2 if i16 else len(x), chunk=chunk, i16=i16)
    assert_same(o.collect(nf), ref, "the call on the checked buffer")
    assert torch.equal(dx, dev(x)), "the stream receiver wrote to its input"


@pytest.mark.parametrize("name", W.WALKER_NAMES)
def test_walker_case(name):
    s = W.walker_streams(name)
    c = s["cfg"]
    x, x16, xd = np.array(s["x"]), np.array(s["x16"]), np.array(s["xd"])
    logt, threads, G, screen, search, nwin = W.expected_walker(c)
    assert W.walker_lds(c) <= W.LDS_LIMIT
    _, small, five = W.chunks(c)
    m = M.Modem(c, 0)
    try:
        def run(samples, **kw):
            return run_guarded(c, samples, m=m, **kw)

        # the three rings, automatic chunks
        ring = run(x)
        want = check_against_oracle(c, x, ring)
        assert len(want) >= 8
        worst = worst_rel_err(c, x, ring)
        cont = run(x, ring=0)
        check_against_oracle(c, x, cont, ring=0)
        tight = run(x, ring=W.small_ring(c))
        check_against_oracle(c, x, tight, ring=W.small_ring(c))
        # chunks: the walk is the same walk, and a frame's decode does not depend on the list it is in
        chunked = run(x, chunk=small)
        check_against_oracle(c, x, chunked)
        assert_same(chunked, ring, "chunks of 1.3 frames")
        stitched = run(x, chunk=small, tuning=dict(lookback=0))
        check_against_oracle(c, x, stitched)
        assert_same(stitched, ring, "chunks of 1.3 frames, host-stitched")
        assert_same(run(x, chunk=five), ring, "chunks of 5 frames")
        check_against_oracle(c, x, run(x, chunk=small, ring=0), ring=0)
        # the other tiers of the scan and of the search
        tunings = [dict(exact_search=1), dict(pre_f32=0)] + ([dict(t2_f32=0)] if screen else [])
        for tuning in tunings:
            other = run(x, chunk=small, tuning=tuning)
            assert_same(other, chunked, f"{tuning}")
            check_against_oracle(c, x, other)
        # the wire format of the same stream
        ref16 = run(xd, chunk=small)
        got16 = run(x16, chunk=small, i16=True)
        assert_same(got16, ref16, "int16 against f64 on the converted samples")
        assert len(check_against_oracle(c, xd, ref16)) >= 8
        worst = max(worst, worst_rel_err(c, xd, ref16))
        # the capture: every zero block goes from the FP32 screen to FP64
        cap, cap16 = (np.array(a) for a in W.capture(c["t2sin_size"]))
        for r in (None, 0):
            f64 = run(cap, ring=r)
            assert len(check_against_oracle(c, cap, f64, ring=r)) >= 4
            assert_same(run(cap16, ring=r, i16=True), f64, f"capture, ring {r}: int16 against f64")
            assert_same(run(cap, ring=r, chunk=small), f64, f"capture, ring {r}: chunks of 1.3 frames")
        assert_input_untouched(m, c, x, False, chunked, small)
        assert_input_untouched(m, c, x16, True, got16, small)
        for a, b in ((x, s["x"]), (x16, s["x16"]), (cap, W.capture(c["t2sin_size"])[0])):
            assert same_bits(a, b)
        print(f"{name}: LOGT {logt}, {threads} threads, G {G}, screen {screen}, {search} x{nwin}, "
              f"{len(want)} frames, worst constellation rel_err {worst:.2e}, "
              f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs")
    finally:
        m.close()


@pytest.mark.parametrize("name", W.WALKER_NAMES)
def test_preamble_search_ends_at_its_last_lag(name):
    """A frame whose first passing lag is among the search's last (the last,
    partial window of the FFT search; lag C - 1 itself where that window
    holds one lag) is located; one whose first passing lag is C or just past
    it (inside the last window, were it taken whole) is not: the walk moves
    on by a message, as the reference's does."""
    c = W.walker_config(*W.WALKER[name])
    msg = O.geometry(c)["message_len"]
    m = M.Modem(c, 0)
    try:
        for where in W.EDGES:
            e = W.edge_stream(name, where)
            if e is None:
                continue
            x = np.array(e["x"])
            got = run_guarded(c, x, ring=0, m=m)
            want = check_against_oracle(c, x, got, ring=0)
            if where == "in":
                assert want.tolist() == [e["lag"] + 1]
            else:
                assert len(want) == 0 or c["t2sin_size"] > msg
            for tuning in (dict(exact_search=1), dict(pre_f32=0), dict(lookback=0)):
                assert_same(run_guarded(c, x, ring=0, tuning=tuning, m=m), got, f"{where}: {tuning}")
    finally:
        m.close()


@pytest.mark.parametrize("name", W.DECODE_NAMES)
def test_decode_case(name):
    s = W.decode_streams(name)
    c = s["cfg"]
    x, x16, xd = np.array(s["x"]), np.array(s["x16"]), np.array(s["xd"])
    assert W.expected_decode(c) == W.DECODE_MEANT[name]
    chunk = 5 * O.geometry(c)["frame_len"]
    m = M.Modem(c, 0)
    try:
        f64 = run_guarded(c, x, chunk=chunk, m=m)
        want = check_against_oracle(c, x, f64)
        assert len(want) >= 4
        got16 = run_guarded(c, x16, chunk=chunk, i16=True, m=m)
        assert len(check_against_oracle(c, xd, got16)) >= 4
        assert_same(run_guarded(c, xd, chunk=chunk, m=m), got16, "int16 against f64 on the converted samples")
        worst = max(worst_rel_err(c, x, f64), worst_rel_err(c, xd, got16))
        if name in W.FUSED_NAMES:
            assert W.expected_decode(c, staged_decode=True) == W.FUSED_STAGED
            for samples, conv, fused, i16 in ((x, x, f64, False), (x16, xd, got16, True)):
                staged = run_guarded(c, samples, chunk=chunk, i16=i16, tuning=dict(staged_decode=1), m=m)
                check_against_oracle(c, conv, staged)
                assert staged[0] == fused[0]
                for part, k in (("pb", 1), ("bytes", 2), ("cfo", 4)):
                    assert same_bits(staged[k], fused[k]), f"staged decode: {part} differs from the fused run"
                assert rel_err(staged[3], fused[3]) < 1e-9
                worst = max(worst, worst_rel_err(c, conv, staged))
        assert_input_untouched(m, c, x, False, f64, chunk)
        print(f"{name}: {W.DECODE_MEANT[name]}, {len(want)} frames, worst constellation rel_err {worst:.2e}")
    finally:
        m.close()


# ------------------------------------------------------------------ the walker's LDS limit
def shard_status(m, c, dx, n, i16=False):
    """ofdm_rx_stream_shard on the C-ABI over the whole stream, every output
    prefilled: (status, nframes, nlocated, exit state, located, lags, outputs)."""
    o = Outputs(c, MF)
    loc, lag = np.full(MF, -7, np.int64), np.full(MF, 7, np.uint8)
    st, ex = M.WalkState(*m.initial_state()), M.WalkState(55, 66)
    nf, nl = C.c_size_t(123), C.c_size_t(456)
    rc = M.lib().ofdm_rx_stream_shard(m.h, None if i16 else dx.data_ptr(), dx.data_ptr() if i16 else None, n,
                                      C.byref(st), 0, n, MF, 0, o.pbs.data_ptr(), o.out.data_ptr(),
                                      o.cons.data_ptr(), o.cfo.data_ptr(), C.byref(nf), loc.ctypes.data,
                                      lag.ctypes.data, MF, C.byref(nl), C.byref(ex), None)
    return rc, nf.value, nl.value, (ex.pos, ex.ring_end), loc, lag, o


@pytest.mark.parametrize("name", list(W.REFUSED))
def test_stream_call_refuses_a_walker_that_does_not_fit(name):
    """OFDM_ERR_UNSUPPORTED with *nframes_out = 0 and the exit state {-1, 0},
    no output touched; the message names the sizes and the bytes; a call on
    another context and the detectors of the refused one still work."""
    size, length = W.REFUSED[name]
    c = W.walker_config(size, length)
    base = W.walker_streams("T2048-L449")
    x, x16 = np.array(base["x"]), np.array(base["x16"])
    m = M.Modem(c, 0)
    try:
        for samples, i16 in ((x, False), (x16, True)):
            dx = dev(samples)
            rc, nf, nl, ex, loc, lag, o = shard_status(m, c, dx, len(x), i16)
            assert rc == ERR_UNSUPPORTED and nf == 0 and nl == 0 and ex == (-1, 0)
            assert np.all(loc == -7) and np.all(lag == 7)
            o.collect(0)  # every output is all sentinel
            fn = m.rx_stream_i16 if i16 else m.rx_stream
            with pytest.raises(M.OfdmError) as e:
                fn(dx, len(x), MF, pb_out=o.pbs, bytes_out=o.out, constell_out=o.cons, cfo_out=o.cfo)
            assert e.value.code == ERR_UNSUPPORTED and "T2sin_size" in str(e.value)
            if size <= 2048:
                assert f"T2sin_size = {size}" in str(e.value) and f"pr_sin_len = {length}" in str(e.value)
                assert str(W.walker_lds(c)) in str(e.value)
            o.collect(0)
            assert torch.equal(dx, dev(samples))
        # another context's stream call is not disturbed
        y = impaired_stream(D, 10, seed=21)[0]  # the stream of test_stream_edges
        assert len(check_against_oracle(D, y, run_guarded(D, y, m=modem(D)))) >= 4
        # the refused context's detectors answer: find_preamble up to pr_sin_len = 664 at 2048, t2_scan at 4096
        dx = dev(x)
        if size <= 2048:
            hit = O.find_t2sin(c, x, 0)
            starts = np.array([hit, hit - 5, 0], np.int32)
            idx = torch.full((3,), 77, dtype=torch.int32, device="cuda")
            m.find_preamble(dx, len(x), dev(starts), 3, idx)
            want = [O.find_preamble(c, x, int(st)) for st in starts]
            assert host(idx).tolist() == want and any(w != -10 for w in want)
        else:
            first = torch.full((1,), 77, dtype=torch.int32, device="cuda")
            m.t2_scan(dx, len(x), 0, first_out=first)
            assert int(host(first)[0]) == O.find_t2sin(c, x, 0)
    finally:
        m.close()
