"""The stream receiver's batched decode, phase timing and walker profiling.

A list longer than one decode launch's scratch (256 MB) is decoded in batches,
and then not speculatively: the host waits for the located list and decodes a
known one (the kernels' `count == nullptr` branches, the offsets `f0` into the
list and into every output). No test stream is that long, so the test hook
OFDM_DECODE_BATCH_FRAMES=<n> caps the frames per launch through the production
formula (batch_frames in ofdm_stream_call.cpp). Each case compares its hooked
run twice: with the oracle's sequential walk and decode
(check_against_oracle: list, CFO and bytes exact, constellation 1e-9), and bit
for bit with the same call with the hook unset (a batch changes which launch a
frame is in, not its arithmetic). Every output buffer of a hooked run carries
sentinels past the frames found and past max_frames.

Then ofdm_set/get_stream_timing (outputs unchanged, values bounded by the
host's wall time, the documented failures), and OFDM_WALK_PROF (the
diagnostics instantiation of the walker walks the same walk; its file has one
well-formed line per walk launch, and none where there is no diagnostics
walker)."""
import ctypes as C
import functools
import json
import math
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle as O
from common import B, D, impaired_stream, rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402
from test_gpu_stream import (check_against_oracle, dev, frame_at, host, modem, run_stream,  # noqa: E402
                             run_stream_i16, to_i16, want_walk)

HOOK = "OFDM_DECODE_BATCH_FRAMES"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADF = 2                            # sentinel frames past max_frames
S_PB, S_BYTE, S_F = -77, 77, 9.0    # fills of pb / bytes / constellation and CFO
MF = 64                             # max_frames above every stream's frame count
INVALID = -1                        # OFDM_ERR_INVALID

D_S12 = dict(D, num_symb=12)        # past the rx register window: the gathered back end
D_CP0 = dict(D, cp_size=0)          # launch_stream_decode answers "not supported": the staged kernels
D_T512 = dict(D, t2sin_size=512, t2_sin_f1=34, t2_sin_f2=102)  # a T2 size without a diagnostics walker


@functools.lru_cache(maxsize=None)
def stream(name):
    """The streams of this file, generated once and left unchanged."""
    if name == "D":        # >= 20 frames located (test_stream_config4_matches_sequential_walk)
        return impaired_stream(D, 40, seed=4)[0]
    if name == "D_long":   # 40 frames in long silences: past 2048 chunks of 256 samples
        return impaired_stream(D, 40, seed=4, gap_max=20000)[0]
    if name == "D10":      # the stream of test_stream_capture_starting_inside_a_frame
        return impaired_stream(D, 10, seed=21)[0]
    if name == "D_gaps":   # the stream of test_stream_lookback_overflow_falls_back_to_halo_walk
        return impaired_stream(D, 40, seed=5, gap_max=6000)[0]
    if name == "D_cp0":
        return impaired_stream(D_CP0, 16, seed=25)[0]
    if name == "D_s12":    # >= 6 frames located (test_stream_unfused_decode_path)
        return impaired_stream(D_S12, 12, seed=5)[0]
    if name == "D_T512":
        return impaired_stream(D_T512, 12, seed=4)[0]
    if name == "B":        # >= 5 frames located (test_stream_wide_fused_decode_matches_oracle_and_staged)
        return impaired_stream(B, 10, seed=21)[0]
    if name in ("B_i16", "D_i16"):  # wire samples as test_stream_wide_fused_decode_i16_equals_f64 makes them
        x = impaired_stream(B, 10, seed=22)[0] if name == "B_i16" else stream("D")
        return to_i16(x * 200.0)
    raise KeyError(name)


def as_f64(x16):
    return x16[0::2].astype(np.float64) + 1j * x16[1::2].astype(np.float64)


class Outputs:
    """One call's output buffers, max_frames + PADF frames each, filled with sentinels."""

    def __init__(self, cfg, max_frames):
        g = O.geometry(cfg)
        self.mf, self.cap = max_frames, max_frames + PADF
        self.pbs = torch.full((self.cap,), S_PB, dtype=torch.int64, device="cuda")
        self.out = torch.full((self.cap * g["bytes_per_frame"],), S_BYTE, dtype=torch.uint8, device="cuda")
        self.cons = torch.full((self.cap * g["npts"],), complex(S_F, S_F), dtype=torch.complex128, device="cuda")
        self.cfo = torch.full((self.cap,), S_F, dtype=torch.float64, device="cuda")

    def collect(self, nf, cons=True, cfo=True):
        """(nf, pb, bytes, constellation, cfo) of the frames written, as
        run_stream returns them, after checking that nothing past them was
        written (a buffer the call did not get must be untouched)."""
        k = min(nf, self.mf)
        pbs, out, = host(self.pbs), host(self.out).reshape(self.cap, -1)
        hc, hf = host(self.cons).reshape(self.cap, -1), host(self.cfo)
        assert np.all(pbs[k:] == S_PB), "pb_out written past the frames found"
        assert np.all(out[k:] == S_BYTE), "bytes_out written past the frames found"
        assert np.all(hc[k if cons else 0:].view(np.float64) == S_F), "constell_out written past the frames found"
        assert np.all(hf[k if cfo else 0:] == S_F), "cfo_out written past the frames found"
        return nf, pbs[:k], out[:k], hc[:k], hf[:k]


class settings:
    """Walk tuning and ring of a context for the length of a `with` block."""

    def __init__(self, m, tuning=None, ring=None):
        self.m, self.tuning, self.ring = m, tuning, ring

    def __enter__(self):
        self.old_t = self.m.walk_tuning(**self.tuning) if self.tuning else None
        self.old_r = self.m.stream_ring(self.ring) if self.ring is not None else None

    def __exit__(self, *exc):
        if self.old_r is not None:
            self.m.stream_ring(self.old_r)
        if self.old_t is not None:
            self.m.walk_tuning(**self.old_t)


def call(m, o, dx, n, chunk=0, i16=False, cons=True, cfo=True, stream=None):
    fn = m.rx_stream_i16 if i16 else m.rx_stream
    return fn(dx, n, o.mf, pb_out=o.pbs, bytes_out=o.out, constell_out=o.cons if cons else None,
              cfo_out=o.cfo if cfo else None, chunk=chunk, stream=stream)


def run_guarded(cfg, x, max_frames=MF, chunk=0, tuning=None, ring=None, i16=False, cons=True, cfo=True, m=None):
    """run_stream with sentinel-filled outputs (x: complex128 samples, or
    interleaved int16 with i16)."""
    m = m or modem(cfg)
    with settings(m, tuning, ring):
        o = Outputs(cfg, max_frames)
        nf = call(m, o, dev(x), len(x) // 2 if i16 else len(x), chunk, i16, cons, cfo)
        return o.collect(nf, cons, cfo)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_run(got, ref):
    """Bit for bit: frame count, pb list, bytes, constellation and (where the
    reference has it) CFO."""
    assert got[0] == ref[0]
    for name, a, b in zip(("pb", "bytes", "constellation", "cfo"), got[1:], ref[1:]):
        assert same_bits(a, b), f"{name} differs from the run with {HOOK} unset"


_refs = {}


def reference(monkeypatch, key, fn):
    """The run with the hook unset, computed once per key."""
    monkeypatch.delenv(HOOK, raising=False)
    if key not in _refs:
        _refs[key] = fn()
    return _refs[key]


def hooked(monkeypatch, batch):
    monkeypatch.setenv(HOOK, str(batch))


def assert_batches_mean_something(nf, batches):
    """More than two batches of every size, and a last batch that is not full
    for at least one."""
    assert all(nf > 2 * b for b in batches), (nf, batches)
    assert any(nf % b for b in batches), (nf, batches)


# ------------------------------------------------------------------ look-back walk
@pytest.mark.parametrize("ring", [None, 0], ids=["ring", "continuous"])
@pytest.mark.parametrize("batch", [1, 3, 4, "nf"])
def test_lookback_fused_decode_of_a_known_list_in_batches(batch, ring, monkeypatch):
    """finish_lookback's non-speculative branch into decode_fused with
    d_cnt == nullptr, N = 512 (launch_stream_decode): batches of 1, 3 and 4
    frames (f0 > 0; the stream has 39 frames, so 4 leaves a last batch that
    is not full), and one batch of exactly the frames found (a known list in
    one launch)."""
    x = stream("D")
    ref = reference(monkeypatch, ("D", ring), lambda: run_stream(D, x, max_frames=MF, chunk=9000, ring=ring))
    nf = ref[0]
    assert_batches_mean_something(nf, (1, 3, 4))
    assert nf < MF  # a batch of nf frames is below the upper bound of the speculative decode: not speculative
    hooked(monkeypatch, nf if batch == "nf" else batch)
    got = run_guarded(D, x, chunk=9000, ring=ring)
    check_against_oracle(D, x, got, ring=ring)
    assert_same_run(got, ref)


def test_lookback_batches_stop_at_max_frames(monkeypatch):
    """max_frames = 5 below the frames found, batches of 2: two full batches
    and one frame, and nothing past five frames is written."""
    x = stream("D")
    ref = reference(monkeypatch, "D_mf5", lambda: run_stream(D, x, max_frames=5, chunk=9000))
    hooked(monkeypatch, 2)
    got = run_guarded(D, x, max_frames=5, chunk=9000)
    assert_same_run(got, ref)
    nf, pbs, out, cons, cfo = got
    want = want_walk(D, x)
    assert nf == len(want) > 5 and np.array_equal(pbs, want[:5])  # every frame reported, five decoded
    g = O.geometry(D)
    for f in range(5):
        c, oc, ob = O.decode_frame(D, frame_at(x, want[f], g["preamble_len"] + g["message_len"]))
        assert cfo[f] == c and rel_err(cons[f], oc) < 1e-9 and np.array_equal(out[f], ob)


@pytest.mark.parametrize("name,cfg,tuning", [("staged_decode", D, dict(staged_decode=1)), ("cp0", D_CP0, None)])
def test_lookback_staged_kernels_in_batches(name, cfg, tuning, monkeypatch):
    """The cfo -> params -> rx kernels on a known list in batches of 3: by
    the tuning, and where launch_stream_decode answers "not supported"."""
    x = stream("D" if cfg is D else "D_cp0")
    ref = reference(monkeypatch, name, lambda: run_stream(cfg, x, max_frames=MF, chunk=9000, tuning=tuning))
    assert_batches_mean_something(ref[0], (3, 4))
    for batch in (3, 4):
        hooked(monkeypatch, batch)
        got = run_guarded(cfg, x, chunk=9000, tuning=tuning)
        assert_same_run(got, ref)
    check_against_oracle(cfg, x, got)


@pytest.mark.parametrize("batch", [1, 4])
def test_lookback_wide_decode_in_batches(batch, monkeypatch):
    """Config B (N = 2048): stream_decode_wide_kernel on a known list."""
    x = stream("B")
    ref = reference(monkeypatch, "B", lambda: run_stream(B, x, max_frames=MF, chunk=40000))
    assert_batches_mean_something(ref[0], (1, 4))
    hooked(monkeypatch, batch)
    got = run_guarded(B, x, chunk=40000)
    check_against_oracle(B, x, got)
    assert_same_run(got, ref)


def test_lookback_wide_decode_i16_in_batches(monkeypatch):
    """The wide kernel's int16 instantiation on a known list, batches of 4."""
    x16 = stream("B_i16")
    ref = reference(monkeypatch, "B_i16", lambda: run_stream_i16(B, x16, max_frames=MF, chunk=40000))
    assert_batches_mean_something(ref[0], (4,))
    hooked(monkeypatch, 4)
    got = run_guarded(B, x16, chunk=40000, i16=True)
    assert_same_run(got, ref)  # the reference run has no CFO output; the oracle pins it
    check_against_oracle(B, as_f64(x16), got)


# ------------------------------------------------------------------ halo walk
@pytest.mark.parametrize("batch", [1, 3, 4])
def test_halo_walk_without_speculative_decode(batch, monkeypatch, capfd):
    """lookback = 0 with the hook: finish_halo launches no compaction and
    decode_stitched decodes every frame."""
    x = stream("D")
    t = dict(lookback=0)
    ref = reference(monkeypatch, "D_halo", lambda: run_stream(D, x, max_frames=MF, chunk=9000, tuning=t))
    assert_batches_mean_something(ref[0], (1, 3, 4))
    hooked(monkeypatch, batch)
    monkeypatch.setenv("OFDM_STREAM_DEBUG", "1")
    capfd.readouterr()
    got = run_guarded(D, x, chunk=9000, tuning=t)
    assert "speculative off" in capfd.readouterr().err
    check_against_oracle(D, x, got)
    assert_same_run(got, ref)


def rewalks(err):
    return [int(n) for n in re.findall(r"(\d+) re-walks", err)]


def test_halo_walk_with_a_rewalk_in_batches(monkeypatch, capfd):
    """No walk-in halo and 5000-sample chunks: the stitch re-walks chunks.
    Unhooked, the speculative list misses and the host's list is decoded over
    it; hooked, the same list is decoded alone, in batches of 3."""
    x = stream("D")
    t = dict(lookback=0, halo_milli=0)
    monkeypatch.delenv(HOOK, raising=False)
    monkeypatch.setenv("OFDM_STREAM_DEBUG", "1")
    capfd.readouterr()
    ref = run_stream(D, x, max_frames=MF, chunk=5000, tuning=t)
    err = capfd.readouterr().err
    assert "speculative miss" in err and rewalks(err)[0] > 0
    assert_batches_mean_something(ref[0], (3, 4))
    for batch in (3, 4):
        hooked(monkeypatch, batch)
        got = run_guarded(D, x, chunk=5000, tuning=t)
        err = capfd.readouterr().err
        assert "speculative off" in err and rewalks(err)[0] > 0
        assert_same_run(got, ref)
    check_against_oracle(D, x, got)


# ------------------------------------------------------------------ gathered back end
@pytest.mark.parametrize("lookback", [1, 0], ids=["lookback", "host_stitch"])
@pytest.mark.parametrize("batch", [1, 4, 5])
def test_gathered_decode_in_batches(batch, lookback, monkeypatch):
    """num_symb = 12: decode_gathered's batches (gather, staged sync chain,
    staged rx; the constellation offset counts doubles, 2 * f0 * npts). The
    stream has 12 frames: batches of 5 leave a last one that is not full."""
    x = stream("D_s12")
    t = dict(lookback=lookback)
    ref = reference(monkeypatch, ("D_s12", lookback),
                    lambda: run_stream(D_S12, x, max_frames=MF, chunk=20000, tuning=t))
    assert_batches_mean_something(ref[0], (1, 4, 5))
    hooked(monkeypatch, batch)
    got = run_guarded(D_S12, x, chunk=20000, tuning=t)
    check_against_oracle(D_S12, x, got)
    assert_same_run(got, ref)


@pytest.mark.parametrize("lookback", [1, 0], ids=["lookback", "host_stitch"])
@pytest.mark.parametrize("cut0", [-200, -3000])
def test_capture_cut_inside_first_frame_in_batches(cut0, lookback, monkeypatch):
    """A capture that starts inside its first frame (in its preamble, in its
    message), walked from the ring's zero header, decoded in batches of 1 and
    2. On these captures the oracle's walk drops the cut frame and locates no
    preamble before sample 0 (nor on any cut of -2 .. -1400 tried on the
    CPU), so decode_list's gathered decode of a prefix (neg > 0) stays
    unreached; what runs is the fused decode of a known list from a walk that
    started in the header."""
    x = stream("D10")
    first = int(want_walk(D, x)[0])
    y = x[first - cut0:]
    t = dict(lookback=lookback)
    ref = reference(monkeypatch, ("cut", cut0, lookback), lambda: run_stream(D, y, max_frames=MF, tuning=t))
    assert_batches_mean_something(ref[0], (1, 2))
    for batch in (1, 2):
        hooked(monkeypatch, batch)
        got = run_guarded(D, y, tuning=t)
        assert_same_run(got, ref)
    check_against_oracle(D, y, got)


# ------------------------------------------------------------------ optional outputs, shards, state
def test_batches_without_cfo_and_constellation_outputs(monkeypatch):
    """cfo_out = NULL (the internal CFO scratch is reused by every batch) and
    constell_out = NULL: the pb list and the bytes of the full-output run."""
    x = stream("D")
    ref = reference(monkeypatch, ("D", None), lambda: run_stream(D, x, max_frames=MF, chunk=9000))
    assert_batches_mean_something(ref[0], (3, 4))
    for batch, cons, cfo in ((3, False, False), (4, False, False), (3, True, False), (3, False, True)):
        hooked(monkeypatch, batch)
        got = run_guarded(D, x, chunk=9000, cons=cons, cfo=cfo)
        assert got[0] == ref[0] and same_bits(got[1], ref[1]) and same_bits(got[2], ref[2])
        assert not cons or same_bits(got[3], ref[3])
        assert not cfo or same_bits(got[4], ref[4])


def shard_call(m, dx, n, own_lo, own_hi, chunk, located_cap=MF):
    """ofdm_rx_stream_shard on the C-ABI from the initial state: every output
    whole (sentinels included), the located list and the exit state."""
    o = Outputs(D, MF)
    loc = np.full(located_cap, -7, np.int64)
    lag = np.full(located_cap, 7, np.uint8)
    st, ex = M.WalkState(*m.initial_state()), M.WalkState()
    nf, nl = C.c_size_t(), C.c_size_t()
    M.check(M.lib().ofdm_rx_stream_shard(m.h, dx.data_ptr(), None, n, C.byref(st), own_lo, own_hi, MF, chunk,
                                         o.pbs.data_ptr(), o.out.data_ptr(), o.cons.data_ptr(), o.cfo.data_ptr(),
                                         C.byref(nf), loc.ctypes.data, lag.ctypes.data, located_cap, C.byref(nl),
                                         C.byref(ex), None))
    got = o.collect(nf.value)
    return dict(run=got, nlocated=nl.value, loc=loc, lag=lag, exit=(ex.pos, ex.ring_end))


@pytest.mark.parametrize("lookback", [1, 0], ids=["lookback", "host_stitch"])
def test_shard_call_in_batches(lookback, monkeypatch):
    """One shard call that owns the stream's last four fifths, located list
    requested, in batches of 3: outputs, located, nlocated and exit state of
    the unhooked call; the owned frames are the oracle's in the owned range."""
    x = stream("D")
    n, own_lo = len(x), len(x) // 5
    m = modem(D)
    dx = dev(x)
    with settings(m, dict(lookback=lookback)):
        monkeypatch.delenv(HOOK, raising=False)
        ref = shard_call(m, dx, n, own_lo, n, 9000)
        hooked(monkeypatch, 3)
        got = shard_call(m, dx, n, own_lo, n, 9000)
    assert_batches_mean_something(ref["run"][0], (3,))
    assert_same_run(got["run"], ref["run"])
    assert got["nlocated"] == ref["nlocated"] > 0 and got["exit"] == ref["exit"]
    assert np.array_equal(got["loc"], ref["loc"]) and np.array_equal(got["lag"], ref["lag"])
    want = want_walk(D, x)
    assert np.array_equal(got["run"][1], want[want >= own_lo])
    whole = reference(monkeypatch, ("D", None), lambda: run_stream(D, x, max_frames=MF, chunk=9000))
    k = len(want) - got["run"][0]  # the owned frames are the whole-stream call's last ones, bit for bit
    for a, b in zip(got["run"][1:], whole[1:]):
        assert same_bits(a, b[k:])


@pytest.mark.parametrize("name,chunk", [("D", 9000), ("D_long", 256)])
def test_state_across_hooked_and_default_calls(name, chunk, monkeypatch, tmp_path, capfd):
    """One context, one stream, no host sync between the calls: hooked
    look-back, default, hooked halo walk, default. The non-speculative
    finishes leave the chunk counter and the publish words to the next call's
    memset (queue_zero / pub_zero), the speculative ones clear them on the
    device; every call equals the reference, and no look-back call falls back
    to the halo walk. The walkers read the chunk counter only where the
    chunks outnumber them: the long-gap stream in 256-sample chunks has more
    chunks than a launch has workgroups (the profiling line's grid shows it)."""
    x = stream(name)
    ref = reference(monkeypatch, (name, chunk), lambda: run_stream(D, x, max_frames=MF, chunk=chunk))
    check_against_oracle(D, x, ref)
    m = modem(D)
    dx = dev(x)
    if name == "D_long":
        path = str(tmp_path / "prof.jsonl")
        monkeypatch.setenv("OFDM_WALK_PROF", path)
        assert_same_run(run_guarded(D, x, chunk=chunk), ref)
        monkeypatch.delenv("OFDM_WALK_PROF")
        line = prof_lines(path)[0]
        assert line["grid"] < line["nchunks"] == -(-len(x) // chunk)
    outs = [Outputs(D, MF) for _ in range(8)]
    torch.cuda.synchronize()
    assert_batches_mean_something(ref[0], (3, 4))
    steps = [(3, None), (None, None), (4, dict(lookback=0)), (None, None)] * 2
    monkeypatch.setenv("OFDM_STREAM_DEBUG", "1")
    capfd.readouterr()
    nfs = []
    for o, (batch, tuning) in zip(outs, steps):
        if batch:
            monkeypatch.setenv(HOOK, str(batch))
        else:
            monkeypatch.delenv(HOOK, raising=False)
        with settings(m, tuning):
            nfs.append(call(m, o, dx, len(x), chunk=chunk))
    for o, nf in zip(outs, nfs):
        assert_same_run(o.collect(nf), ref)
    err = capfd.readouterr().err
    assert "look-back overflow" not in err and err.count("look-back,") == 6 and err.count("speculative off") == 2


@pytest.mark.parametrize("value", ["0", "-3", "abc", "3x", ""])
def test_hook_values_that_are_ignored(value, monkeypatch, capfd):
    """Not an integer >= 1: as unset, so the halo walk decodes speculatively."""
    x = stream("D")
    t = dict(lookback=0)
    ref = reference(monkeypatch, "D_halo", lambda: run_stream(D, x, max_frames=MF, chunk=9000, tuning=t))
    monkeypatch.setenv(HOOK, value)
    monkeypatch.setenv("OFDM_STREAM_DEBUG", "1")
    capfd.readouterr()
    got = run_guarded(D, x, chunk=9000, tuning=t)
    assert "speculative hit" in capfd.readouterr().err
    assert_same_run(got, ref)


# ------------------------------------------------------------------ phase timing
def timing_code(m):
    w, r, d = C.c_float(), C.c_float(), C.c_float()
    return M.lib().ofdm_get_stream_timing(m.h, C.byref(w), C.byref(r), C.byref(d))


def timed_call(m, cfg, dx, n, chunk):
    """(run, wall ms): the call between two device syncs on the host's clock."""
    o = Outputs(cfg, MF)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nf = call(m, o, dx, n, chunk=chunk)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return o.collect(nf), wall


def assert_times_valid(m, wall):
    t = m.last_stream_times()
    vals = (t["walk_ms"], t["resolve_ms"], t["decode_ms"])
    assert all(math.isfinite(v) and v > 0 for v in vals), t
    # the three phases lie end to end inside the call: the device cannot have
    # spent longer in them than the host waited for the call and the stream
    assert sum(vals) <= wall, (t, wall)
    return vals


def test_stream_timing_outputs_values_and_documented_failures(monkeypatch):
    """A fresh context: ofdm_get_stream_timing fails until a timed look-back
    call with a speculative decode has run, and again after every call that
    is not one; a timed call's outputs are the untimed call's."""
    x = stream("D")
    ref = reference(monkeypatch, ("D", None), lambda: run_stream(D, x, max_frames=MF, chunk=9000))
    dx = dev(x)
    m = M.Modem(D, 0)
    try:
        assert timing_code(m) == INVALID                 # before any timed call
        run, _ = timed_call(m, D, dx, len(x), 9000)      # timing off: still none
        assert_same_run(run, ref)
        assert timing_code(m) == INVALID
        m.stream_timing(True)
        assert timing_code(m) == INVALID                 # switched on, no call yet
        run, wall = timed_call(m, D, dx, len(x), 9000)
        assert_same_run(run, ref)
        first = assert_times_valid(m, wall)
        run, wall = timed_call(m, D, dx, len(x), 9000)   # a second timed call: fresh values, same outputs
        assert_same_run(run, ref)
        second = assert_times_valid(m, wall)
        assert second != first  # microsecond-resolution floats of two runs: stale values would repeat all three

        def untimed(tuning=None, batch=None):
            """From a state with valid times: a call that takes none."""
            monkeypatch.delenv(HOOK, raising=False)
            run, wall = timed_call(m, D, dx, len(x), 9000)
            assert_times_valid(m, wall)
            if batch:
                hooked(monkeypatch, batch)
            with settings(m, tuning):
                run, _ = timed_call(m, D, dx, len(x), 9000)
            monkeypatch.delenv(HOOK, raising=False)
            assert_same_run(run, ref)
            assert timing_code(m) == INVALID
            with pytest.raises(M.OfdmError) as e:
                m.last_stream_times()
            assert e.value.code == INVALID

        untimed(tuning=dict(lookback=0))      # the halo walk
        untimed(batch=3)                      # look-back whose decode is not speculative
        untimed(tuning=dict(max_rec_cap=1))   # look-back that overflowed into the halo walk
        m.stream_timing(False)                # switched off, then a call
        assert timing_code(m) == INVALID
        run, _ = timed_call(m, D, dx, len(x), 9000)
        assert_same_run(run, ref)
        assert timing_code(m) == INVALID
    finally:
        m.close()


def test_stream_timing_argument_checks_and_other_t2_size(monkeypatch):
    lib = M.lib()
    m = M.Modem(D_T512, 0)
    try:
        f = C.c_float()
        for on in (2, -1):
            assert lib.ofdm_set_stream_timing(m.h, on) == INVALID
        assert lib.ofdm_set_stream_timing(None, 1) == INVALID
        assert lib.ofdm_get_stream_timing(None, C.byref(f), C.byref(f), C.byref(f)) == INVALID
        # timing on a context with T2sin_size = 512 works like any other
        x = stream("D_T512")
        monkeypatch.delenv(HOOK, raising=False)
        dx = dev(x)
        ref, _ = timed_call(m, D_T512, dx, len(x), 20000)
        assert ref[0] >= 4
        m.stream_timing(True)
        run, wall = timed_call(m, D_T512, dx, len(x), 20000)
        assert_same_run(run, ref)
        assert_times_valid(m, wall)
        for args in ((None, C.byref(f), C.byref(f)), (C.byref(f), None, C.byref(f)), (C.byref(f), C.byref(f), None)):
            assert lib.ofdm_get_stream_timing(m.h, *args) == INVALID  # NULL outputs, valid times or not
        check_against_oracle(D_T512, x, run)
    finally:
        m.close()


# ------------------------------------------------------------------ OFDM_WALK_PROF
def prof_lines(path):
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def check_prof_line(d, n, chunk, lookback):
    """One line of the file against the call that wrote it."""
    assert d["chunk"] == chunk and d["nchunks"] == -(-n // chunk) and d["lookback"] == lookback
    fields, rows = d["fields"], d["chunks"]
    assert len(fields) == 14 and len(rows) == d["nchunks"] and 0 < d["grid"] <= d["nchunks"]
    col = {name: i for i, name in enumerate(fields)}
    for row in rows:
        assert len(row) == len(fields)
        r = {name: row[i] for name, i in col.items()}
        assert 0 < r["t0"] <= r["t_end"], r
        assert 0 <= r["block"] < d["grid"] and 0 <= r["xcc"] < 8, r
        assert r["nrec"] >= 0 and r["searches"] >= r["nrec"] and r["scan_steps"] >= 0, r
    return sum(row[col["nrec"]] for row in rows)


@pytest.mark.parametrize("lookback", [1, 0], ids=["lookback", "host_stitch"])
@pytest.mark.parametrize("fmt", ["f64", "i16"])
def test_walk_prof_walks_the_same_walk(fmt, lookback, monkeypatch, tmp_path):
    """stream_walk_kernel<8, *, true>, the instantiation every walker timeline
    comes from, against the product's: every output bit for bit, and one
    well-formed line for the call's one walk launch."""
    i16 = fmt == "i16"
    x = stream("D_i16") if i16 else stream("D")
    n = len(x) // 2 if i16 else len(x)
    t = dict(lookback=lookback)
    monkeypatch.delenv(HOOK, raising=False)
    monkeypatch.delenv("OFDM_WALK_PROF", raising=False)
    ref = run_guarded(D, x, chunk=9000, tuning=t, i16=i16)
    path = str(tmp_path / "prof.jsonl")
    monkeypatch.setenv("OFDM_WALK_PROF", path)
    got = run_guarded(D, x, chunk=9000, tuning=t, i16=i16)
    assert_same_run(got, ref)
    check_against_oracle(D, as_f64(x) if i16 else x, got)
    lines = prof_lines(path)
    assert len(lines) == 1
    assert check_prof_line(lines[0], n, 9000, lookback) >= got[0]  # every frame found is in some walker's records


def test_walk_prof_overflow_writes_two_lines_and_the_summary_tool_reads_them(monkeypatch, tmp_path, capfd):
    """max_rec_cap = 1: the look-back walk overflows and the halo walk takes
    the call, one line each. tools/walk_prof_summary.py summarises the file."""
    x = stream("D_gaps")
    t = dict(max_rec_cap=1)
    monkeypatch.delenv(HOOK, raising=False)
    ref = run_guarded(D, x, chunk=9000, tuning=t)
    path = str(tmp_path / "prof.jsonl")
    monkeypatch.setenv("OFDM_WALK_PROF", path)
    monkeypatch.setenv("OFDM_STREAM_DEBUG", "1")
    capfd.readouterr()
    got = run_guarded(D, x, chunk=9000, tuning=t)
    assert "look-back overflow" in capfd.readouterr().err
    assert_same_run(got, ref)
    lines = prof_lines(path)
    assert [d["lookback"] for d in lines] == [1, 0]
    for d, lookback in zip(lines, (1, 0)):
        check_prof_line(d, len(x), 9000, lookback)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "walk_prof_summary.py"), path],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert [c["lookback"] for c in json.loads(r.stdout)["calls"]] == [1, 0]


def test_walk_prof_rewalk_adds_no_line(monkeypatch, tmp_path, capfd):
    """A host-stitch call whose stitch re-walks chunks: the re-walk is a
    launch of the product's walker and writes no line. (run_stream, without
    sentinels: on a speculative miss the compaction's longer list has been
    written to the outputs past the frames found, inside max_frames, before
    the host's list is decoded over it.)"""
    x = stream("D")
    t = dict(lookback=0, halo_milli=0)
    monkeypatch.delenv(HOOK, raising=False)
    ref = run_stream(D, x, max_frames=MF, chunk=5000, tuning=t)
    path = str(tmp_path / "prof.jsonl")
    monkeypatch.setenv("OFDM_WALK_PROF", path)
    monkeypatch.setenv("OFDM_STREAM_DEBUG", "1")
    capfd.readouterr()
    got = run_stream(D, x, max_frames=MF, chunk=5000, tuning=t)
    assert rewalks(capfd.readouterr().err)[0] > 0
    assert_same_run(got, ref)
    lines = prof_lines(path)
    assert len(lines) == 1
    check_prof_line(lines[0], len(x), 5000, 0)


@pytest.mark.parametrize("lookback", [1, 0], ids=["lookback", "host_stitch"])
def test_walk_prof_without_a_diagnostics_walker_writes_no_line(lookback, monkeypatch, tmp_path):
    """T2sin_size = 512 has no diagnostics instantiation: the normal walker
    runs and would leave the timeline buffer unwritten. The call succeeds with
    the unprofiled outputs and the file gets no line (tools/README.md)."""
    x = stream("D_T512")
    t = dict(lookback=lookback)
    monkeypatch.delenv(HOOK, raising=False)
    monkeypatch.delenv("OFDM_WALK_PROF", raising=False)
    ref = run_guarded(D_T512, x, chunk=20000, tuning=t)
    assert ref[0] >= 4
    path = str(tmp_path / "prof.jsonl")
    monkeypatch.setenv("OFDM_WALK_PROF", path)
    got = run_guarded(D_T512, x, chunk=20000, tuning=t)
    assert_same_run(got, ref)
    assert not os.path.exists(path) or os.path.getsize(path) == 0
