"""The fixtures of tests/test_gpu_rx_geometry.py (tests/rx_geometry_cases.py),
checked on the CPU with the oracle alone: the launches the GPU module makes
reach every non-stream instance of rx_kernel and rx_soft_kernel, the few-frame
kernel at every size it is built for and the six body branches the table aims
at; every case is a geometry the library accepts; and on every case's input
the oracle round-trips the payload, keeps every point clear of its decision
edges (so the GPU's bytes can be asked to be bit-exact) and, from 16-QAM on,
decides some bits wrong (so the error counter has something to count).
Without that the GPU test could pass blind."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import rx_geometry_cases as RG

NUM_CUS = 256  # the MI355X; the GPU module asserts the same rule with the device's own count


def launches(num_cus):
    out = []
    for name in RG.NAMES:
        c = RG.CASES[name]
        for entry, nf, i16, soft, with_chan in RG.runs(name, num_cus):
            inst = RG.expected_instance(c, nf, i16, soft, num_cus)
            out.append((name, entry, nf, inst, RG.body_branches(c, inst, with_chan)))
    return out


def test_launches_cover_every_instance_and_branch():
    got = launches(NUM_CUS)
    for name in RG.NAMES:  # every launch takes the instance the table means it for
        for entry, nf, i16, soft, _ in RG.runs(name, NUM_CUS):
            assert RG.expected_instance(RG.CASES[name], nf, i16, soft, NUM_CUS) == RG.meant_instance(
                name, nf, i16, soft), (name, entry, nf)
    assert set(RG.WIDE_CASES) <= set(RG.NAMES)
    instances = {inst for _, _, _, inst, _ in got}
    want = {(fam, logn, staged, i16) for fam in ("rx_kernel", "rx_soft_kernel") for logn in range(6, 13)
            for staged in (False, True) for i16 in (False, True)}
    assert len(want) == 56
    wide = {("rx_wide_kernel", logn, False, False) for logn in range(9, 13)}
    assert want - instances == set(), "rx_kernel / rx_soft_kernel instances no launch reaches"
    assert wide - instances == set(), "rx_wide_kernel instances no launch reaches"
    assert instances == want | wide
    branches = set().union(*(b for _, _, _, _, b in got))
    assert branches == set(RG.BRANCHES) and len(RG.BRANCHES) == 6
    # the branches by the launches that take them: each by a hard and by a soft launch where both have it
    by = {b: {entry for _, entry, _, _, br in got if b in br} for b in RG.BRANCHES}
    assert by["chan_lds false with a channel"] == {"rx_read"}
    for b in RG.BRANCHES:
        if b != "chan_lds false with a channel":
            assert {"rx", "rx_i16", "rx_soft"} <= by[b], (b, by[b])
    # chan_lds false both with the whole frame's decisions in LDS and with one symbol's
    dec = {RG.whole_frame_dec(RG.CASES[n]) for n, e, _, _, br in got if "chan_lds false with a channel" in br}
    assert dec == {True, False}
    # the few-frame kernel is taken at FEW frames alone, and by the channel launch as well
    for name, entry, nf, inst, _ in got:
        if inst[0] == "rx_wide_kernel":
            assert nf == RG.FEW and entry in ("rx", "rx_read")
        if nf != RG.FEW:
            assert inst[0] == "rx_kernel" and nf > NUM_CUS // 2
    assert {e for _, e, _, inst, _ in got if inst[0] == "rx_wide_kernel"} == {"rx", "rx_read"}
    # from N = 512 on a case that fits the window and is not the few-frame kernel's at FEW frames either
    assert any(inst == ("rx_kernel", 11, False, False) and nf == RG.FEW for _, _, nf, inst, _ in got)


def test_rule_follows_the_device():
    """The few-frame kernel needs nframes <= CUs / 2: a part with 4 CUs takes the persistent kernel at 3 frames."""
    c = RG.CASES["N1024-D328-P8-cp3-k6-S4"]
    assert RG.expected_instance(c, 3, False, False, 256) == ("rx_wide_kernel", 10, False, False)
    assert RG.expected_instance(c, 3, False, False, 4) == ("rx_kernel", 10, False, False)
    assert RG.expected_instance(c, 130, False, False, 256) == ("rx_kernel", 10, False, False)
    assert RG.expected_instance(c, 3, True, False, 256) == ("rx_kernel", 10, False, True)
    assert RG.expected_instance(c, 3, False, True, 256) == ("rx_soft_kernel", 10, False, False)
    # S * T > 1024 threads, or frames that do not fit the LDS: not the few-frame kernel's
    assert not RG.rx_wide_ok(RG.CASES["N2048-D8-P2-cp0-k2-S8"], 3, 256)
    assert RG.rx_wide_shm(dict(c, fft_size=4096, num_symb=2)) > RG.LDS_LIMIT


def test_cases_are_geometries_the_library_accepts():
    import ofdm_mi355x as M
    for name, c in RG.CASES.items():
        N, D, P, k = c["fft_size"], c["num_data_subc"], c["num_pilot_subc"], c["mod_type"]
        assert P % 2 == 0 and D % P == 0 and D % 8 == 0 and (D * k) % 8 == 0 and D <= N // 2, name
        assert P <= min(N // 8, 256) and RG.layout_ok(N, D, P), name
        assert RG.valid(c) and RG.rx_shm(c) <= RG.LDS_LIMIT, name
        pil, seg = O.layout(N, D, P)  # the oracle's layout: inside [1, N) as well
        assert pil.min() >= 1 and pil.max() < N and seg.min() >= 1 and seg.max() + D // P <= N, name
        # validate() itself: ofdm_create gets past it (to the device check, where there is no GPU)
        h = C.c_void_p()
        prm = M.Params.make(**c)
        rc = M.lib().ofdm_create(C.byref(prm), 0, C.byref(h))
        assert rc in (0, -3), (name, rc)
        if rc == 0:
            M.lib().ofdm_destroy(h)
    # an odd pilot count puts a pilot at bin N: validate() refuses it (never fed to the oracle)
    odd = dict(O.DEFAULT, num_data_subc=224, num_pilot_subc=7)
    assert not RG.valid(odd) and not RG.layout_ok(512, 224, 7)
    h = C.c_void_p()
    assert M.lib().ofdm_create(C.byref(M.Params.make(**odd)), 0, C.byref(h)) == -1
    # the geometry edges the table is there for
    cs = RG.CASES.values()
    assert {1, 0} <= {c["cp_size"] for c in cs} and any(c["cp_size"] == c["fft_size"] for c in cs)
    assert sum(c["cp_size"] % 2 for c in cs) >= 5
    assert any(c["num_pilot_subc"] == 2 and c["num_data_subc"] < c["fft_size"] // 8 for c in cs)
    assert any(c["num_pilot_subc"] == c["fft_size"] // 8 for c in cs)
    assert any(c["fft_size"] // 8 - 2 <= c["num_pilot_subc"] < c["fft_size"] // 8 for c in cs)
    assert any(c["num_data_subc"] % 64 and c["fft_size"] >= 512 for c in cs)
    assert {c["mod_type"] for c in cs} == {1, 2, 4, 6, 8}
    # lanes masked (D < N/2) in staged launches and at every T
    assert {c["fft_size"] for c in cs if c["num_data_subc"] < c["fft_size"] // 2} == {64, 128, 256, 512, 1024, 2048,
                                                                                      4096}
    assert {c["fft_size"] for c in cs if c["num_data_subc"] < c["fft_size"] // 2 and not RG.fits(c)} >= {256, 512,
                                                                                                          4096}


@pytest.mark.parametrize("name", RG.NAMES)
def test_oracle_alone_behaves(name):
    c = RG.CASES[name]
    g = O.geometry(c)
    k, bpf = c["mod_type"], g["bytes_per_frame"]
    for nf in RG.frame_counts(c, NUM_CUS):
        x = RG.inputs(name, nf)
        stride, msg = x["stride"], g["message_len"]
        assert stride == msg + 3 and len(x["iq"]) == nf * stride
        gaps = x["iq"].reshape(nf, stride)[:, msg:]
        assert np.isnan(gaps.real).all() and not np.isnan(x["iq"].reshape(nf, stride)[:, :msg]).any()
        _, back, errs = O.rx_batch(c, x["clean"], nf, stride, ref=x["data"], threads=8)
        assert np.array_equal(back, x["data"]) and errs == 0, "the oracle does not round-trip the payload"
        assert not np.isnan(x["cons"]).any()
        print(f"{name} x{nf}: closest point {x['edge']:.2e} from a decision edge, "
              f"{RG.bit_errors(x['bytes'], x['data'])} bit errors")
        assert x["edge"] >= RG.EDGE_BAR
        if k >= 4:
            assert RG.bit_errors(x["bytes"][:RG.FEW * bpf], x["data"][:RG.FEW * bpf]) > 0
        assert RG.bit_errors(x["bytes"], x["ref"]) > nf * bpf  # the reference the GPU counts against: not the payload
        if nf != RG.FEW:  # the first frames do not depend on the count
            few = RG.inputs(name, RG.FEW)
            assert np.array_equal(few["iq"].view(np.uint64), x["iq"][:RG.FEW * stride].view(np.uint64))
            assert np.array_equal(few["bytes"], x["bytes"][:RG.FEW * bpf])
            assert np.array_equal(few["ref"], x["ref"][:RG.FEW * bpf])
            ch = RG.channel(name, nf)
            assert np.array_equal(RG.channel(name, RG.FEW), ch[:RG.FEW * c["num_data_subc"]])
    # the wire-format input
    w = RG.i16_input(name)
    x16 = w["x16"].reshape(RG.FEW, stride, 2)
    assert np.all(x16[:, msg:] == RG.GAP_I16)
    assert 100 < w["peak"] < 8192, "the scaled samples use the format without coming near its ends"
    for pos, v in zip(RG.extreme_positions(c), RG.EXTREMES):
        assert tuple(x16[1, pos]) == v and c["cp_size"] <= pos % g["symbol_len"] and pos < msg
    assert len(set(RG.extreme_positions(c))) == 4
    assert np.abs(x16[[0, 2], :msg].astype(np.int32)).max() <= w["peak"]
    print(f"{name} int16: closest point {w['edge']:.2e} from a decision edge, largest |int16| {w['peak']}")
    assert w["edge"] >= RG.EDGE_BAR and not np.isnan(w["cons"]).any()
    # the samples are the f64 input's, scaled and truncated; the extremes change four samples of frame 1
    body = RG.inputs(name, RG.FEW)["iq"].reshape(RG.FEW, stride)[:, :msg] * c["mult"]
    differ = (np.trunc(body.real) != x16[:, :msg, 0]) | (np.trunc(body.imag) != x16[:, :msg, 1])
    assert differ.sum() == differ[1].sum() == 4
    assert np.array_equal(w["iq"].real, w["x16"][0::2]) and np.array_equal(w["iq"].imag, w["x16"][1::2])
