"""The fixtures of tests/test_gpu_t2_near_level.py, checked on the CPU with the
oracle alone: every crafted block's longdouble detector ratio is where the
case says (level + delta; int16 blocks, whose rounding moves the
ratio by a few 1e-7: the delta reached, within 10 % of the target), and the oracle's walk differs between +delta and -delta of every pair
(one frame when the block passes, two when it fails). Without that the GPU
test would be blind to the decision it is about."""
import numpy as np
import pytest

import oracle as O
import t2_level_cases as T


@pytest.mark.parametrize("key", list(T.CONFIGS))
def test_the_located_frames_reveal_the_decision(key):
    cfg, G = T.CONFIGS[key]
    cases = T.cases(key)
    level = T.level_of(cfg)
    assert len(cases) == 2 * len(T.MAGS) * (2 * G + 2)
    for c in cases:
        got = float(c["ratio"] - T.dt.LD(level))
        tol = 0.1 * abs(c["delta"]) if c["scale"] == "int16" else 1e-9
        assert abs(got - c["delta"]) <= tol, (c["pair"], c["delta"], got)
        assert len(c["want"]) == (1 if c["delta"] > 0 else 2), (c["pair"], c["delta"], c["want"])
    for up, down in zip(cases[0::2], cases[1::2]):
        assert up["pair"] == down["pair"] and up["delta"] == -down["delta"] > 0
        assert np.array_equal(up["want"], down["want"][1:])  # the first frame is the one lost
    # every slot of the first scan step and two of the second; every texture, scale and background with both signs
    assert {c["slot"] for c in cases} == set(range(2 * G)) | {2 * G + 1, 3 * G}
    seen = {(c["texture"], c["scale"], c["fill"]) for c in cases}
    assert len(seen) == len(T.TEXTURES) * len(T.SCALES) * len(T.FILLS)
    assert {(c["slot"], c["fill"]) for c in cases} == {(s, f) for s in {c["slot"] for c in cases} for f in T.FILLS}
    assert O.stream_walk(cfg, cases[0]["x"]).tolist() == cases[0]["want"].tolist()
