"""The constants of a modem context on the CPU: c-ofdm_amd/apps/tables_selftest.cpp
writes every table of csrc/ofdm_tables.hpp (what ofdm_create and cfo_plan
upload), built with the host's address and undefined-behaviour sanitizers, and
each one is compared here with the oracle: integers exactly, the FP64 tables
at test_gpu_parity.py's tolerance, the template spectrum against an FFT."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from common import cfg, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "c-ofdm_amd", "bin", "tables_selftest")
TOL = 1e-10          # tests/test_gpu_parity.py TOL: both sides FP64
WALK_FFT_M = 512     # csrc/ofdm_sync.hpp
# the smallest supported geometry; the comb fits: pilots at bins 9, 18, 46, 55
N64 = cfg(O.DEFAULT, fft_size=64, num_data_subc=32, num_pilot_subc=4, cp_size=16, t2sin_size=64, pr_sin_len=32)
CONFIGS = {"D": O.DEFAULT, "B": O.CONFIG_B, "C": O.CONFIG_C, "N64": N64}
CFO_NSYM = (1, 9)


@pytest.fixture(scope="module")
def selftest():
    subprocess.run(["make", "-C", os.path.join(ROOT, "c-ofdm_amd"), "bin/tables_selftest"], check=True,
                   capture_output=True)
    return SELFTEST


def run(exe, c, out_dir, preamble):
    pre = os.path.join(out_dir, "preamble_in.f64")
    np.ascontiguousarray(preamble, np.complex128).tofile(pre)
    args = [str(c[f]) for f in O.PARAM_FIELDS] + [str(out_dir), pre] + [str(n) for n in CFO_NSYM]
    return subprocess.run([exe] + args, capture_output=True, text=True)


@pytest.fixture(scope="module")
def tables(selftest, tmp_path_factory):
    """name -> (config, the oracle's preamble_setup, a reader of the selftest's files)"""
    out = {}
    for name, c in CONFIGS.items():
        d = tmp_path_factory.mktemp(name)
        setup = O.preamble_setup(c)
        r = run(selftest, c, d, setup[0])
        assert r.returncode == 0 and "tables_selftest: ok" in r.stdout, r.stdout + r.stderr
        kinds = {"i32": np.int32, "u32": np.uint32, "i64": np.int64, "u8": np.uint8, "f64": np.float64,
                 "c64": np.complex128}

        def read(fname, kind=None, d=d):
            return np.fromfile(os.path.join(d, fname), kinds[kind or fname.rsplit(".", 1)[1]])
        out[name] = (c, setup, read)
    return out


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_geometry_and_layout(tables, name):
    c, _, read = tables[name]
    N, D, P = c["fft_size"], c["num_data_subc"], c["num_pilot_subc"]
    seg = D // P
    g, og = read("geometry.i64"), O.geometry(c)
    got = dict(zip(["symbol_len", "message_len", "preamble_len", "frame_len", "ring_len", "data_per_frame",
                    "bytes_per_frame", "segment_size"], g.tolist()))
    for key in ("symbol_len", "message_len", "preamble_len", "frame_len", "data_per_frame", "bytes_per_frame"):
        assert got[key] == og[key], key
    # ofdm_mi355x.h: ring_len = frame_len * (rx_buf_size + 1), segment_size = D / P
    assert got["ring_len"] == og["frame_len"] * (c["rx_buf_size"] + 1) and got["segment_size"] == seg
    opil, oseg = O.layout(N, D, P)
    pilot, segst = read("pilot.i32"), read("segst.i32")
    assert np.array_equal(pilot, opil) and np.array_equal(segst, oseg)
    if name == "N64":
        assert pilot.tolist() == [9, 18, 46, 55]
    # the tables derived from the layout, from their definitions
    data_bin = (oseg[:, None] + np.arange(seg)[None, :]).ravel()
    data_slot = np.repeat(np.arange(P), seg)
    bin_map = np.full(N, -1, np.int32)
    bin_map[opil] = -2
    bin_map[data_bin] = np.arange(D)
    assert np.array_equal(read("data_bin.i32"), data_bin) and np.array_equal(read("data_slot.i32"), data_slot)
    assert np.array_equal(read("bin_map.i32"), bin_map)
    assert np.count_nonzero(bin_map == -1) == N - D - P and bin_map[0] == -1

    def swz(e):  # csrc/ofdm_fft.hpp lds_swz
        return e ^ ((e >> 3) & 7)
    rx_pack = np.zeros(max(D, 4 * (N // 8)), np.int32)
    rx_pack[:D] = swz(data_bin) | (data_slot << 16)
    pilot_swz = np.zeros(max(P, N // 8), np.int32)
    pilot_swz[:P] = swz(opil)
    assert np.array_equal(read("rx_pack.i32"), rx_pack) and np.array_equal(read("pilot_swz.i32"), pilot_swz)
    # csrc/ofdm_internal.hpp: tx_code_data, tx_code_fixed(TX_LDS_PILOT = 256 / TX_LDS_ZERO = 257), tx_dead_masks
    tx_code = np.where(bin_map >= 0, bin_map | (0xff << 13), np.where(bin_map == -2, 256 << 21, 257 << 21))
    assert np.array_equal(read("tx_code.i32"), tx_code)
    T = N // 8
    dead = [sum(1 << i for i in range(8) if np.all(bin_map[64 * w + T * i: 64 * w + T * i + 64] == -1))
            for w in range(T // 64)]
    assert read("tx_dead.u32").tolist() == dead


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_constellations_t2_and_preamble(tables, name):
    c, (opre, omodp, otempl), read = tables[name]
    for k in (1, 2, 4, 6, 8):
        assert rel_err(read(f"constellation_{k}.f64", "c64"), O.constellation(k)) < TOL, k
    assert rel_err(read("t2_symbol.f64", "c64"), O.t2_symbol(c)) < TOL
    t2, sm = c["t2sin_size"], c["smooth"]
    mask = np.zeros(t2)
    for f in (c["t2_sin_f1"], c["t2_sin_f2"]):
        mask[max(0, f - sm): min(t2 - 1, f + sm) + 1] += 1.0
    assert np.array_equal(read("t2_mask.f64"), mask)
    assert np.array_equal(read("preamble_bytes.u8"), O.preamble_bytes(c))
    assert np.array_equal(read("mod_preamble.f64", "c64"), omodp)
    assert rel_err(read("templ.f64", "c64"), otempl) < TOL


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_template_spectrum(tables, name):
    """tspec_k = sum_j c_j e^{+2 pi i k j / M} = M * ifft of the zero-padded
    template. The template has unit energy and at most M - 63 taps: a double
    FFT of it errs by about eps log2(M) = 2.4e-15, the long double sum by the
    final rounding of a value of at most sqrt(M - 63); 1e-13 absolute is well
    above both and far below any indexing error."""
    c, _, read = tables[name]
    templ = read("templ.f64", "c64")
    assert len(templ) == c["pr_sin_len"] <= WALK_FFT_M - 63
    padded = np.zeros(WALK_FFT_M, np.complex128)
    padded[: len(templ)] = templ
    want = WALK_FFT_M * np.fft.ifft(padded)
    got = read("tspec.f64", "c64")
    assert got.shape == want.shape
    err = np.abs(got - want).max()
    print(f"{name}: template spectrum max abs err {err:.3e}")
    assert err < 1e-13
    assert read("tspec_max.f64")[0] == np.hypot(got.real, got.imag).max()


def test_layout_that_does_not_fit(selftest, tmp_path):
    # N = 64, D = 60, P = 4: both halves of the comb claim bin 32
    c = cfg(N64, num_data_subc=60)
    r = run(selftest, c, tmp_path, np.zeros(80, np.complex128))
    assert r.returncode != 0
    assert "pilot comb does not fit fft_size" in r.stdout + r.stderr


def test_cfo_plan_borders(tables):
    """pilot_freq_sinh's window borders on the default geometry, against
    Frame.hpp:311-321 written out here; a form of 1 symbol (640 = 5 * 2^7
    samples) has a kernel, one of 9 symbols (5760) has none."""
    c, _, read = tables["D"]
    N, D, P = c["fft_size"], c["num_data_subc"], c["num_pilot_subc"]
    for nsym, shape in zip(CFO_NSYM, ((5, 7), (0, -1))):
        S = (N + c["cp_size"]) * nsym
        rel_bw = float(D + P) / N
        rel_pilot_w = rel_bw / P
        pilot_w = int(S * rel_pilot_w)
        j = int((1.0 - rel_bw - rel_pilot_w) / 2.0 * S)
        borders = []
        for _ in range(P + 2):
            borders.append(j)
            j += pilot_w
        borders[0] = max(0, borders[0])
        got = read(f"cfo_{nsym}.i32")
        assert tuple(got[:2]) == shape, nsym
        assert got[2:].tolist() == borders, nsym
