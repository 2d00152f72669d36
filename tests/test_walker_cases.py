"""The fixtures of tests/test_gpu_walker_geometry.py (tests/walker_cases.py),
checked on the CPU with the oracle alone: the walker table reaches every
stream_walk_kernel size, both preamble searches and the window counts it is
there for, inside the walker's LDS limit; the decode table reaches the narrow
fused kernel, the staged stream kernels at N = 64, 128, 256 and 4096 and the
five CFO instances no other stream test launches; and on every stream the
oracle's own walk finds enough frames, crosses ring ends, and keeps every
point of every located frame clear of its decision edges (so the GPU's bytes
can be asked to be bit-exact); the edge streams put their first passing lag
where they say, and the oracle locates the one inside the search's range and
not the one past it. Without that the GPU test could pass blind."""
import numpy as np
import pytest

import oracle as O
import walker_cases as W
from rx_geometry_cases import valid

# a capture has CAPTURE_FRAMES = 8 frames and no noise; the T2 search on the
# ring's grid misses some of them, as the reference's does, so the bar of the
# 12-frame streams (8) cannot hold: half of the frames, the decode table's bar
CAPTURE_MIN = 4


def test_walker_table_reaches_every_instance_search_and_window_count():
    assert len(W.WALKER) == 15
    got = {name: W.expected_walker(W.walker_config(*W.WALKER[name])) for name in W.WALKER_NAMES}
    assert {e[0] for e in got.values()} == set(range(6, 12))
    for logt in (6, 8, 10):
        assert {e[4] for e in got.values() if e[0] == logt} == {"fft", "direct"}
    nwin = {e[5] for e in got.values() if e[4] == "fft"}
    assert 1 in nwin and nwin & {2, 3} and max(nwin) == 72 and sum(w >= 10 for w in nwin) >= 3
    # WalkShape: 128 threads and G = 1024 / T2sin_size blocks per step; 256 threads at 2048
    assert {(e[0], e[1], e[2]) for e in got.values()} == {(6, 128, 16), (7, 128, 8), (8, 128, 4), (9, 128, 2),
                                                          (10, 128, 1), (11, 256, 1)}
    assert {e[0] for e in got.values() if e[3]} == {6, 7, 8, 9}  # the FP32 screen
    # a full last window, and partial ones down to one lag
    last = {name: W.windows(W.walker_config(*W.WALKER[name]))[-1] for name in W.WALKER_NAMES if got[name][4] == "fft"}
    assert min(last.values()) == 1 and any(1 < v < 512 + 1 - W.WALKER[n][1] for n, v in last.items())
    for name, e in got.items():
        assert e[5] == len(W.windows(W.walker_config(*W.WALKER[name]))) or e[4] == "direct"
        print(name, e, W.walker_lds(W.walker_config(*W.WALKER[name])), W.WALKER_AIMS[name])


def test_walker_lds_limit():
    for name in W.WALKER_NAMES:
        assert W.walker_lds(W.walker_config(*W.WALKER[name])) <= W.LDS_LIMIT, name
    # WalkLds<11> by hand: FIXED = 16 (96 + 4) + 64 + 16 + 128 + 16 * 72, direct = 131088 + 72 L
    assert W.walker_lds(W.walker_config(2048, 450)) == 2960 + 131088 + 72 * 450 == 166448
    assert W.walker_lds(W.walker_config(2048, 640)) > W.LDS_LIMIT
    with pytest.raises(ValueError):
        W.walker_lds(W.walker_config(4096, 128))
    # T2sin_size = 2048 has no direct search: the direct form would fit up to L = 413, where the FFT search runs
    direct = lambda length: 2960 + 131088 + 72 * length  # noqa: E731
    assert direct(413) <= W.LDS_LIMIT < direct(414) and 413 <= W.FFT_L_MAX
    assert W.walker_lds(W.walker_config(2048, W.FFT_L_MAX)) <= W.LDS_LIMIT
    # the limits the header states for the smaller sizes
    for size, most in ((1024, 1328), (512, 1785)):
        assert W.walker_lds(W.walker_config(size, most)) <= W.LDS_LIMIT < W.walker_lds(W.walker_config(size, most + 1))


def test_decode_table_reaches_the_kernels_it_names():
    assert len(W.DECODE) == 10 and len(W.FUSED_NAMES) == 5
    for name, c in W.DECODE.items():
        assert valid(c) and W.fused_geometry(c), name
        assert W.expected_decode(c) == W.DECODE_MEANT[name], name
    for name in W.FUSED_NAMES:
        assert W.expected_decode(W.DECODE[name], staged_decode=True) == W.FUSED_STAGED
    staged = [m for m in W.DECODE_MEANT.values() if m[0] == "staged"]
    assert {m[1] for m in staged} == {6, 7, 8, 12}
    assert {m[2] for m in staged} == {(6, 1), (7, 1), (8, 1), (6, 5), (12, 1)}
    # the narrow kernel's bounds: S 1 and 8, P 2 and near 64, D 8 and no multiple of 64, every modulation
    f = [W.DECODE[n] for n in W.FUSED_NAMES]
    assert {c["num_symb"] for c in f} >= {1, 8} and {c["num_pilot_subc"] for c in f} >= {2, 62, 64}
    assert {c["mod_type"] for c in f} == {1, 2, 4, 6, 8} and any(c["num_data_subc"] % 64 for c in f)
    # the rule itself on configs outside the table
    assert W.expected_decode(O.DEFAULT) == ("fused-narrow",)
    assert W.expected_decode(O.CONFIG_B) == ("fused-wide", 11) and W.expected_decode(O.CONFIG_C) == ("fused-wide", 12)
    assert W.expected_decode(dict(O.DEFAULT, num_symb=12)) == ("gathered",)
    assert W.expected_decode(dict(O.DEFAULT, cp_size=0)) == ("staged", 9, (9, 1), "rx_stream2")


def check_stream(c, x, ring, least, ring_ends):
    pbs, crossed = W.walk(c, x, ring)
    edge = W.edge_distance(c, x, pbs)
    assert len(pbs) >= least and crossed >= ring_ends and edge >= W.EDGE_BAR, (len(pbs), crossed, edge)
    return pbs, edge


@pytest.mark.parametrize("name", W.WALKER_NAMES)
def test_walker_streams_are_well_conditioned(name):
    s = W.walker_streams(name)
    c = s["cfg"]
    assert c["rx_buf_size"] == 3 and c["num_symb"] == 2 and 55000 <= len(s["x"]) <= 80000
    for key in ("x", "xd"):
        ring = check_stream(c, s[key], None, 8, 2)
        cont = check_stream(c, s[key], 0, 8, 0)
        small = check_stream(c, s[key], W.small_ring(c), 8, 2)
        print(f"{name} {key}: {len(ring[0])} / {len(cont[0])} / {len(small[0])} frames (ring, continuous, small "
              f"ring), closest point {min(ring[1], cont[1], small[1]):.2e} from a decision edge")
    assert np.array_equal(s["xd"].real, s["x16"][0::2]) and np.array_equal(s["xd"].imag, s["x16"][1::2])
    assert 100 < np.abs(s["x16"].astype(np.int32)).max() < 8192  # the format is used without coming near its ends
    cap, cap16 = W.capture(c["t2sin_size"])
    assert np.array_equal(cap.real, cap16[0::2]) and np.count_nonzero(cap == 0) > len(cap) // 10
    for ring in (None, 0):
        pbs, edge = check_stream(c, cap, ring, CAPTURE_MIN, 2 if ring is None else 0)
        print(f"{name} capture ring {ring}: {len(pbs)} frames, closest point {edge:.2e}")


def test_ring_and_continuous_walks_differ():
    differ = [name for name in W.WALKER_NAMES
              if not np.array_equal(W.walk(W.walker_streams(name)["cfg"], W.walker_streams(name)["x"], None)[0],
                                    W.walk(W.walker_streams(name)["cfg"], W.walker_streams(name)["x"], 0)[0])]
    assert differ, "the ring never changes the walk: rx_buf_size = 3 tests nothing"
    print("ring walk != continuous walk on", differ)


@pytest.mark.parametrize("name", W.DECODE_NAMES)
def test_decode_streams_are_well_conditioned(name):
    s = W.decode_streams(name)
    c = s["cfg"]
    assert 27000 <= len(s["x"]) <= 155000
    for key in ("x", "xd"):
        pbs, edge = check_stream(c, s[key], None, 4, 0)
        print(f"{name} {key}: {len(pbs)} frames, closest point {edge:.2e} from a decision edge")


@pytest.mark.parametrize("name", W.WALKER_NAMES)
def test_edge_streams_put_the_first_passing_lag_where_they_say(name):
    c = W.walker_config(*W.WALKER[name])
    cyc = 2 * c["t2sin_size"] + c["pr_sin_len"]
    msg = O.geometry(c)["message_len"]
    for where in W.EDGES:
        e = W.edge_stream(name, where)
        if e is None:  # "out" needs a partial last window
            assert where == "out" and W.windows(c)[-1] == 512 + 1 - c["pr_sin_len"]
            continue
        x, lag = e["x"], e["lag"]
        assert e["range"] == W.edge_range(c, where) and e["range"][0] <= lag <= e["range"][1]
        assert O.find_t2sin(c, x, 0) == 0  # the marker is block 0 of the continuous walk
        pbs = O.stream_walk_ring(c, x, ring=0)[0]
        if where == "in":
            assert lag < cyc and (W.expected_walker(c)[4] == "direct" or lag >= cyc - W.windows(c)[-1])
            assert O.find_preamble(c, x, 0) == lag and pbs.tolist() == [lag + 1]
            assert W.edge_distance(c, x, pbs) >= W.EDGE_BAR
        else:
            assert lag >= cyc and O.find_preamble(c, x, 0) == -10
            # the walk moves on by a message; past a marker longer than that (T2sin_size = 2048) the next
            # search starts inside the marker and reaches the frame: there "out" shows nothing
            assert len(pbs) == 0 or c["t2sin_size"] > msg
        print(f"{name} {where}: first passing lag {lag} in {e['range']} of C = {cyc}, walk {pbs.tolist()}")
    # the table has last windows of one lag, partial ones and the direct search on both sides of the edge
    assert W.edge_stream("T64-L449", "in")["range"] == (576, 576)
