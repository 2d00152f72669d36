"""The real stream walker at the T2 level: ofdm_rx_stream on streams whose one
crafted block has a detector ratio of level + delta, |delta| from a quarter of
the FP32 screen's margin (4e-5) to eight times it (tests/t2_level_cases.py: the
block in every slot of the first FP32 scan step, so in both packed lanes of
every group, and in two slots of the second step; two textures; scales 1e-3,
200 and full-scale int16; f64 and int16 entry points; zero and weak-noise
backgrounds). The located frames reveal the block's decision: one frame when
it passed, two when it failed; tests/test_t2_level_cases.py asserts on the CPU
that the oracle's walk differs between +delta and -delta of every case, and
the same is asserted here.

- Default tuning: the walk and the decoded frames equal the oracle's. The
  FP32 verdict decides for |delta| > margin, the FP64 re-evaluation below it.
- t2_margin = 0 with allow_uncertified (the raw FP32 verdicts): the walk equals
  the oracle's for every |delta| >= 2.5e-5: the model's 2.1e-5 bound on the
  FP32 ratio, on the real kernel. With the weak-noise
  background the crafted block's own FP32 verdict is what the walk acts on.
- Under the same raw tuning every case's decision equals the verdict of the
  devtest replica of the screen (devtest.fft32p) on the same block in the same
  packed lane: the replica, on which tests/test_gpu_walk_bounds.py measures
  the ratio error, is the kernel's arithmetic.
- t2_f32 = 0 (the FP64 scan) gives the same walks."""
import numpy as np
import pytest

import devtest as dt
import oracle as O
import t2_level_cases as T
from common import check_stream_frames

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

RAW = dict(t2_margin=0.0, allow_uncertified=1)
MAX_FRAMES = 8
_m = {}


def modem(key):
    if key not in _m:
        _m[key] = M.Modem(T.CONFIGS[key][0], 0)
    return _m[key]


def walk(key, case, tuning=None, i16=False):
    """ofdm_rx_stream (ring 0: the continuous walk) on one case's stream:
    (pbs, bytes, constellations, cfo or None)."""
    cfg = T.CONFIGS[key][0]
    m, g = modem(key), O.geometry(cfg)
    x = case["x"]
    old_ring = m.stream_ring(0)
    old = m.walk_tuning(**tuning) if tuning else None
    try:
        pbs = torch.full((MAX_FRAMES,), -1, dtype=torch.int64, device="cuda")
        out = torch.zeros((MAX_FRAMES * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
        cons = torch.zeros((MAX_FRAMES * g["npts"],), dtype=torch.complex128, device="cuda")
        cfo = torch.zeros((MAX_FRAMES,), dtype=torch.float64, device="cuda")
        if i16:
            nf = m.rx_stream_i16(torch.from_numpy(T.int16_wire(x)).cuda(), len(x), MAX_FRAMES, pb_out=pbs,
                                 bytes_out=out, constell_out=cons)
        else:
            nf = m.rx_stream(torch.from_numpy(np.array(x)).cuda(), len(x), MAX_FRAMES, pb_out=pbs, bytes_out=out,
                             constell_out=cons, cfo_out=cfo)
        torch.cuda.synchronize()
    finally:
        if old is not None:
            m.walk_tuning(**old)
        m.stream_ring(old_ring)
    assert nf <= MAX_FRAMES
    return (pbs.cpu().numpy()[:nf], out.cpu().numpy().reshape(MAX_FRAMES, -1)[:nf],
            cons.cpu().numpy().reshape(MAX_FRAMES, -1)[:nf], None if i16 else cfo.cpu().numpy()[:nf])


def entries(case):
    """The entry points a case runs through: f64 always, int16 when its stream is integer-valued."""
    return (False, True) if case["scale"] == "int16" else (False,)


def reached(key, case):
    """|ratio - level| of the crafted block, in longdouble."""
    return abs(float(case["ratio"] - dt.LD(T.level_of(T.CONFIGS[key][0]))))


def check_blind_spot(cases):
    for up, down in zip(cases[0::2], cases[1::2]):
        assert len(up["want"]) == 1 and len(down["want"]) == 2  # the oracle's walk reveals the decision


@pytest.mark.parametrize("key", list(T.CONFIGS))
def test_default_tuning_walks_and_decodes_as_the_oracle(key):
    cfg = T.CONFIGS[key][0]
    cases = T.cases(key)
    check_blind_spot(cases)
    for c in cases:
        for i16 in entries(c):
            pbs, out, cons, cfo = walk(key, c, i16=i16)
            assert np.array_equal(pbs, c["want"]), (c["pair"], c["delta"], c["slot"], i16, pbs, c["want"])
            check_stream_frames(cfg, c["x"], pbs, out, cons, cfo, threads=2)


@pytest.mark.parametrize("key", list(T.CONFIGS))
def test_raw_fp32_verdicts_are_right_beyond_the_model_bound(key):
    cfg, G = T.CONFIGS[key]
    cases = T.cases(key)
    check_blind_spot(cases)
    logt = cfg["t2sin_size"].bit_length() - 1
    # the replica's raw verdict of every crafted block, in the packed lane its slot gives it in the walk
    blocks = np.stack([c["block"] for c in cases])
    _, _, _, verdict = dt.fft32p(logt, blocks, blocks, T.mask_of(cfg), T.level_of(cfg), 0.0)
    asserted = 0
    for i, c in enumerate(cases):
        lane = (c["slot"] % (2 * G)) // G
        replica = int(verdict[i, lane])
        assert replica in (0, 1)
        for i16 in entries(c):
            pbs = walk(key, c, tuning=RAW, i16=i16)[0]
            assert len(pbs) in (1, 2) and np.array_equal(pbs, c["want"][-len(pbs):]), (c["pair"], pbs)
            decision = 1 if len(pbs) == 1 else 0
            # (weak-noise background: the block's own FP32 verdict decided; zeros: an FP64 step may have)
            assert decision == replica, (c["pair"], c["delta"], c["slot"], c["fill"], i16, decision, replica)
            if reached(key, c) >= 2.5e-5:
                assert np.array_equal(pbs, c["want"]), (c["pair"], c["delta"], c["slot"], i16, pbs, c["want"])
                asserted += 1
    assert asserted >= len(cases) * 4 // 5  # every |delta| but the smallest


@pytest.mark.parametrize("key", list(T.CONFIGS))
def test_fp64_scan_gives_the_same_walks(key):
    cases = T.cases(key)
    for c in cases:
        for i16 in entries(c):
            pbs = walk(key, c, tuning=dict(t2_f32=0), i16=i16)[0]
            assert np.array_equal(pbs, c["want"]), (c["pair"], c["delta"], c["slot"], i16, pbs, c["want"])
