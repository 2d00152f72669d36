"""The conditioning the non-flat GPU tests rely on, checked on the CPU with
the oracle alone (no GPU): chan_phase_path (tests/common.py) reproduces
O.chan_char_lq, and on every case of the channel tables the unwrap really
adjusts entries, visits all its states, and no compare or decision sits close
enough to its threshold for a rounding difference to flip it. The distances
are conditions on the inputs: a seed that violates one is replaced, the bars
stay."""
import numpy as np
import pytest

import oracle as O
from common import (CHAN_ONLY_CASES, CHANNEL_CASES, STREAM_CASES, channel_frames, chan_phase_path,
                    distance_to_threshold, stream_case_samples, synced_region)

PI_MARGIN = 1e-6     # rad: no unwrap compare closer to +-pi, in any state
EDGE_MARGIN = 1e-7   # no oracle constellation point closer to a decision edge

_cache = {}


def _frame_stats(case):
    """Per frame of a frames case: (restated phase path, oracle chan vector,
    oracle constellation or None where rx refuses the geometry)."""
    name, cfg, taps, offset, seed, nf = case
    if name not in _cache:
        g = O.geometry(cfg)
        modp = O.preamble_setup(cfg)[1]
        regions, _ = channel_frames(cfg, nf, seed, taps, offset)
        out = []
        for r in regions:
            _, s = synced_region(cfg, r)
            pre = s[: g["preamble_len"]]
            cons = O.decode_frame(cfg, r)[1] if cfg["num_data_subc"] <= cfg["fft_size"] // 2 else None
            out.append((chan_phase_path(cfg, pre, modp), O.chan_char_lq(cfg, pre, modp), cons))
        _cache[name] = out
    return _cache[name]


def _stream_stats(case):
    name, cfg = case[:2]
    if name not in _cache:
        g = O.geometry(cfg)
        modp = O.preamble_setup(cfg)[1]
        x, _ = stream_case_samples(case)
        pbs = O.stream_walk_ring(cfg, x)[0]  # the walk the stream tests expect
        n = g["preamble_len"] + g["message_len"]
        assert pbs.min() >= 0 and pbs.max() + n <= len(x)
        out = []
        for pb in pbs:
            r = x[pb: pb + n]
            _, s = synced_region(cfg, r)
            pre = s[: g["preamble_len"]]
            out.append((chan_phase_path(cfg, pre, modp), O.chan_char_lq(cfg, pre, modp), O.decode_frame(cfg, r)[1]))
        _cache[name] = out
    return _cache[name]


FRAME_CASES = CHANNEL_CASES + CHAN_ONLY_CASES
ALL = [(c, _frame_stats) for c in FRAME_CASES] + [(c, _stream_stats) for c in STREAM_CASES]
IDS = [c[0] for c, _ in ALL]


@pytest.mark.parametrize("case,stats", ALL, ids=IDS)
def test_phase_path_restatement_equals_oracle(case, stats):
    """Only a restatement that reproduces the oracle's channel vector may
    count its unwrap adjustments."""
    frames = stats(case)
    assert len(frames) >= (3 if stats is _frame_stats else 7)
    for p, ch, _ in frames:
        assert np.abs(p["chan"] - ch).max() < 1e-9


@pytest.mark.parametrize("case,stats", ALL, ids=IDS)
def test_case_makes_the_unwrap_work_and_is_well_conditioned(case, stats):
    """Every frame of a frames case adjusts entries; in a stream the detector
    may still land on a frame's exact start, so most frames must (3 in 4)."""
    k = case[1]["mod_type"]
    frames = stats(case)
    working = sum(p["adjusted"] > 0 for p, _, _ in frames)
    assert working == len(frames) if stats is _frame_stats else 4 * working >= 3 * len(frames), working
    for f, (p, _, cons) in enumerate(frames):
        assert p["pi_margin"] > PI_MARGIN, f"frame {f}: a compare {p['pi_margin']:.2e} rad from +-pi"
        if cons is not None:
            d = float(distance_to_threshold(k, cons).min())
            assert d > EDGE_MARGIN, f"frame {f}: a point {d:.2e} from a decision edge"


def test_table_visits_every_state_and_changes_state_often():
    states, most = set(), 0
    for case, stats in ALL:
        for p, _, _ in stats(case):
            states |= set(np.unique(p["adjust"]).tolist())
            most = max(most, p["state_changes"])
    assert states == {-1, 0, 1}
    assert most >= 10
