"""The fixtures of tests/test_gpu_tx_geometry.py (tests/tx_cases.py), checked
on the CPU with the oracle alone: every case is a geometry ofdm_create takes;
the launches reach the 35 instances of tx_kernel the C ABI can reach and every
branch value the table aims at, the noisy ones in both emit forms; the
committed AWGN counters have the uniforms they are listed for, O.awgn gives
there what the definition says, and each sample_offset puts its counter where
it claims; the numpy restatement of the counter hash equals O.awgn across a
2^32 boundary; and the oracle's wire samples leave assert_int16_match's
ambiguity band all but empty, so that rule cannot hide a wrong int16 sample.
Without that the GPU test could pass blind."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import tx_cases as TC


def test_cases_are_geometries_the_library_accepts():
    import ofdm_mi355x as M
    for name, c in TC.CASES.items():
        assert TC.valid(c), name
        h = C.c_void_p()
        rc = M.lib().ofdm_create(C.byref(M.Params.make(**c)), 0, C.byref(h))
        assert rc in (0, -3), (name, rc)  # past validate(): to the device check, where there is no GPU
        if rc == 0:
            M.lib().ofdm_destroy(h)
        g = O.geometry(c)
        assert TC.frames_of(name) * g["frame_len"] < 500_000, name  # small launches
    # what the relaxed rule still refuses, and validate() with it
    for bad in (dict(O.DEFAULT, num_data_subc=224, num_pilot_subc=7), dict(O.DEFAULT, num_data_subc=512),
                dict(O.DEFAULT, cp_size=513), dict(O.DEFAULT, mod_type=3)):
        assert not TC.valid(bad)
        h = C.c_void_p()
        assert M.lib().ofdm_create(C.byref(M.Params.make(**bad)), 0, C.byref(h)) in (-1, -2)
    cs = TC.CASES.values()
    assert {c["fft_size"] for c in cs} == {64, 128, 256, 512, 1024, 2048, 4096}
    assert {c["mod_type"] for c in cs} == {1, 2, 4, 6, 8}
    # D > N/2 at k = 8: with and without dead-group forms; D < T
    assert {c["fft_size"] for c in cs if c["num_data_subc"] > c["fft_size"] // 2 and c["mod_type"] == 8} >= {128, 512}
    assert any(c["num_data_subc"] < c["fft_size"] // 8 for c in cs)
    # the payload stage holds N bytes: the fullest case uses all but 8 of them
    assert max(c["num_data_subc"] * c["mod_type"] / 8 / c["fft_size"] for c in cs) == 120 / 128


def test_runs_reach_every_instance_and_branch():
    runs = TC.runs()
    assert len({r[0] for r in runs}) == len(TC.NAMES) and runs == [r for n in TC.NAMES for r in TC.runs(n)]
    inst = {}
    for name, nf, entry, noise, i16, align, std, off in runs:
        assert (std > 0) == noise and (noise or off == 0)
        inst.setdefault(TC.expected_instance(TC.CASES[name], entry, noise, i16), set()).add(entry)
    want = {("tx_kernel", logn, points, noise, i16) for logn in (6, 7, 8, 9, 10, 11, 12)
            for points, noise, i16 in ((False, False, False), (False, False, True), (False, True, False),
                                       (False, True, True), (True, False, False))}
    assert len(want) == 35 and want == TC.INSTANCES == set(inst)
    # the 21 other instantiations (POINTS with NOISE or I16) have no entry point
    c = TC.CASES[TC.EDGE_CASE]
    for entry, noise, i16 in (("fft_write", True, False), ("fft_write", False, True), ("fft_write", True, True),
                              ("tx_frames", True, False)):
        with pytest.raises(ValueError):
            TC.expected_instance(c, entry, noise, i16)
    # ofdm_tx_frames takes <L,0,0,0> and <L,0,0,1> at LOGN 6, 9 and 12
    frames = {i for i, e in inst.items() if "tx_frames" in e}
    assert frames == {("tx_kernel", logn, False, False, i16) for logn in (6, 9, 12) for i16 in (False, True)}

    def reached(pick):
        return set().union(*(TC.branches(TC.CASES[r[0]], r[1], r[5], r[2]) for r in runs if pick(r)))

    every = {"by_word", "bytes: bps % 4", "bytes: bytes_per_frame % 4", "bytes: pointer",
             "cp_reg i_cp=0", "cp_reg i_cp=1", "cp_reg i_cp=6", "cp_reg i_cp=7", "cp_reg i_cp=8", "general cp",
             "DFT8_Z2345", "DFT8_Z34", "full", "no dead-group forms (T < 64)", "masks all 0",
             "nsym > TX_MAX_GRID", "nsym <= TX_MAX_GRID", "gridDim % S != 0", "header"}
    assert every == TC.BRANCHES == reached(lambda r: True)
    # ofdm_tx_modulate meets all of them but the header, noise-free and in each noisy form
    for noise in (False, True):
        for i16 in (False, True):
            got = reached(lambda r: r[2] == "tx" and r[3] == noise and r[4] == i16)
            assert got == every - {"header"}, (noise, i16, every - got)
    # the header: a few frames, and more symbols than the grid with S not dividing it
    assert reached(lambda r: r[2] == "tx_frames") >= {"header", "nsym > TX_MAX_GRID", "gridDim % S != 0",
                                                     "nsym <= TX_MAX_GRID"}
    # ofdm_fft_write: every LOGN, and once past the grid
    assert reached(lambda r: r[2] == "fft_write") >= {"nsym > TX_MAX_GRID", "gridDim % S != 0", "cp_reg i_cp=8",
                                                     "DFT8_Z2345", "DFT8_Z34", "full"}
    assert {TC.CASES[r[0]]["fft_size"] for r in runs if r[2] == "fft_write"} == {64, 128, 256, 512, 1024, 2048, 4096}
    # by_word fails for one cause alone in two launches: bps % 4 (bytes_per_frame a multiple of 4), the pointer
    alone = [TC.branches(TC.CASES[r[0]], r[1], r[5]) & {"bytes: bps % 4", "bytes: bytes_per_frame % 4",
                                                        "bytes: pointer"} for r in runs if r[2] == "tx"]
    assert {"bytes: bps % 4"} in alone and {"bytes: pointer"} in alone
    assert {"bytes: bps % 4", "bytes: bytes_per_frame % 4"} in alone
    # general cp with noise: cp = 1, an odd cp, and cp > T (several trips of the CP loop)
    gen = {TC.CASES[r[0]]["cp_size"] for r in runs if r[3] and "general cp" in TC.branches(TC.CASES[r[0]], r[1], r[5])}
    assert {1, 3, 5, 511, 1023} <= gen
    # the three noise levels in both forms; more than 4096 symbols at N = 64 with S = 7 in both forms
    assert {(r[6], r[4]) for r in runs if r[3]} == {(s, i) for s in (0.3, 1e-6, 50.0) for i in (False, True)}
    big = [r for r in runs if r[3] and r[1] * TC.CASES[r[0]]["num_symb"] > 4096]
    assert {r[4] for r in big} == {False, True}
    assert all(TC.CASES[r[0]]["fft_size"] == 64 and TC.CASES[r[0]]["num_symb"] == 7 for r in big)


def test_dead_masks_of_known_layouts():
    """dead_masks against the masks tests/test_gpu_tx_sparse.py reads back from the library."""
    assert TC.dead_masks(O.DEFAULT) == [0x18]
    assert TC.dead_masks(O.CONFIG_B) == [0x38, 0x3c, 0x3c, 0x1c]
    assert TC.dead_masks(O.CONFIG_C) == [0x38] + [0x3c] * 6 + [0x1c]
    assert TC.dead_masks(dict(O.DEFAULT, num_data_subc=480, num_pilot_subc=16)) == [0]
    assert TC.dead_masks(TC.CASES["N512-D40-P2-cp511-k4-S2"]) == [0x7e]
    assert TC.dead_masks(TC.CASES["N512-D448-P8-cp3-k8-S2"]) == [0]
    assert TC.dead_masks(TC.CASES["N64-D24-P6-cp8-k8-S3"]) == []


def test_edge_counters_have_the_uniforms_they_are_listed_for():
    assert set(TC.EDGE_COUNTERS) == set(TC.EDGE_UNIFORMS)
    for kind, g in TC.EDGE_COUNTERS.items():
        which, top = TC.EDGE_UNIFORMS[kind]
        h1, h2 = TC.awgn_hashes(TC.AWGN_SEED, np.array([g], np.uint64))
        assert int((h1 if which == "h1" else h2)[0]) >> 8 == top, kind
    # the definition at those counters, through the oracle
    for std in (TC.NOISE_STD, TC.NOISE_SMALL, TC.NOISE_LARGE):
        radius = TC.MAX_RADIUS * std / np.sqrt(2.0)
        assert abs(TC.MAX_RADIUS - np.sqrt(2 * 24 * np.log(2.0))) < 1e-15
        # the increments on a zero sample: nothing of them is lost to the sample's rounding
        inc = {kind: complex(O.awgn(np.zeros(1, np.complex128), std, seed=TC.AWGN_SEED, sample_offset=g)[0])
               for kind, g in TC.EDGE_COUNTERS.items()}
        x = complex(0.25, -0.75)
        assert inc["u1_one"] == 0 and O.awgn(np.array([x]), std, seed=TC.AWGN_SEED,
                                             sample_offset=TC.EDGE_COUNTERS["u1_one"])[0] == x
        assert abs(abs(inc["u1_min"]) - radius) < 1e-6 * radius
        for kind, axis in (("u2_0", 1), ("u2_q1", 1j), ("u2_q2", -1), ("u2_q3", -1j)):
            r = abs(inc[kind])
            assert 0 < r < radius and abs(inc[kind] - axis * r) < 1e-6 * r, kind
        for kind, g in TC.EDGE_COUNTERS.items():  # and the restatement
            mine = complex(TC.awgn_noise(TC.AWGN_SEED, np.array([g], np.uint64), std)[0])
            assert abs(mine - inc[kind]) <= 1e-12 * radius, kind


def test_edge_search_finds_the_committed_counters():
    assert TC.edge_search() == TC.EDGE_COUNTERS


def test_sample_offsets_put_the_counters_where_they_claim():
    seen = set()
    for name, nf, kind, where, sym, j in TC.EDGES:
        c = TC.CASES[name]
        L, S = c["fft_size"] + c["cp_size"], c["num_symb"]
        off = TC.edge_offset(c, kind, sym, j)
        assert off + sym * L + j == TC.EDGE_COUNTERS[kind] and 0 <= sym < nf * S
        assert {"first CP sample": j == 0 and c["cp_size"] > 0, "last body sample": j == L - 1}[where]
        assert TC.edge_at(name, off) == [(name, nf, kind, where, sym, j)]
        # the oracle's noise over the launch's contiguous samples has the extreme at that sample and nowhere else
        h1, h2 = TC.awgn_hashes(TC.AWGN_SEED, off + np.arange(nf * S * L, dtype=np.uint64))
        which, top = TC.EDGE_UNIFORMS[kind]
        hits = np.flatnonzero(((h1 if which == "h1" else h2) >> np.uint64(8)) == np.uint64(top))
        assert list(hits) == [sym * L + j]
        for i16 in (False, True):  # both emit forms launch it
            assert (name, nf, "tx", True, i16, 0, TC.NOISE_STD, off) in TC.runs(name)
        seen.add((kind, where, sym >= TC.TX_MAX_GRID))
    for kind in TC.EDGE_COUNTERS:
        assert (kind, "first CP sample", False) in seen and (kind, "last body sample", False) in seen
    assert {(k, w) for k, w, past in seen if past} == {("u1_min", "first CP sample"), ("u1_one", "last body sample")}


def test_hash_restatement_equals_the_oracle_across_a_2_32_boundary():
    n, std = 4096, 0.3
    for hi in (1, 7):
        off = (hi << 32) - n // 2 - 5
        want = O.awgn(np.zeros(n, np.complex128), std, seed=TC.AWGN_SEED, sample_offset=off)
        mine = TC.awgn_noise(TC.AWGN_SEED, off + np.arange(n, dtype=np.uint64), std)
        assert np.abs(mine - want).max() <= 1e-12 * np.abs(want).max()
        # the keys change with the high word: the same low words one period later give other noise
        other = TC.awgn_noise(TC.AWGN_SEED, off + (1 << 32) + np.arange(n, dtype=np.uint64), std)
        assert np.abs(other - want).max() > 0.1


@pytest.mark.parametrize("name", TC.NAMES)
def test_int16_comparisons_are_well_conditioned(name):
    """At most 0.1 % of the components of the oracle's x * mult of every
    noise-free launch lie inside assert_int16_match's band."""
    c = TC.CASES[name]
    g = O.geometry(c)
    for run in TC.runs(name):
        _, nf, entry, noise, i16 = run[:5]
        if not TC.int16_by_oracle(run):
            assert not i16 or noise or (entry, nf) == ("tx_frames", TC.MANY)
            continue
        if entry == "tx":
            x = TC.inputs(name, nf)["clean"]
            assert x.shape == (nf, g["message_len"])
        else:
            assert entry == "tx_frames"
            x = TC.frames_ref(name, nf)
            assert x.shape == (nf, g["frame_len"])
            # the message part of a frame is the batched tx of the same payload
            assert np.array_equal(x[:, g["frame_len"] - g["message_len"]:], TC.inputs(name, nf)["clean"])
        share = TC.int16_band_share(x, c["mult"])
        print(f"{name} {entry} x{nf}: {share * x.size * 2:.0f} of {x.size * 2} components in the band")
        assert share <= TC.INT16_BAND_SHARE
        assert 100 < np.abs(x).max() * c["mult"] < 32767


def test_points_are_off_the_constellation_with_both_zeros():
    for name in TC.NAMES:
        c = TC.CASES[name]
        pts = TC.points(name, TC.FEW)
        assert pts.size == TC.FEW * c["num_symb"] * c["num_data_subc"]
        zero = (pts.real == 0) & (pts.imag == 0)
        neg = zero & np.signbit(pts.real) & np.signbit(pts.imag)
        assert neg.sum() >= 1 and (zero & ~neg).sum() >= 1
        assert not np.isin(pts[~zero], O.constellation(c["mod_type"])).any()
