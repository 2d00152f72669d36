"""Channel-code host arithmetic of the C ABI (no GPU): the exported symbols,
ofdm_fec_coded_bits / ofdm_fec_max_info_bits / ofdm_fec_workspace_size against
tests/fec_model.py, and their error returns."""
import ctypes as C

import pytest

import fec_model as F
import ofdm_mi355x as M
import oracle as O
from common import ALL_CONFIGS

NEW = ("ofdm_fec_coded_bits", "ofdm_fec_max_info_bits", "ofdm_fec_workspace_size", "ofdm_fec_encode",
       "ofdm_fec_decode")


def test_library_exports_the_channel_code():
    L = M.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in M.SIGNATURES
    assert (M.FEC_R12, M.FEC_R23, M.FEC_R34) == (F.R12, F.R23, F.R34)
    for name in ("fec_encode", "fec_decode", "fec_coded_bits", "fec_max_info_bits", "fec_workspace_size"):
        assert hasattr(M.Modem, name)


@pytest.mark.parametrize("rate", F.RATES)
def test_coded_bits_equal_the_model(rate):
    for nb in range(1, 301):
        assert M.fec_coded_bits(nb, rate) == F.coded_bits(nb, rate), nb


@pytest.mark.parametrize("rate", F.RATES)
def test_max_info_bits_equal_the_model(rate):
    for cap in range(F.coded_bits(1, rate), 340):
        assert M.fec_max_info_bits(cap, rate) == F.max_info_bits(cap, rate), cap
    # the frame capacities of the test configs: the largest codeword that fits
    for name, p in ALL_CONFIGS.items():
        cap = O.geometry(p)["bytes_per_frame"] * 8
        nb = M.fec_max_info_bits(cap, rate)
        assert F.coded_bits(nb, rate) <= cap < F.coded_bits(nb + 1, rate), name
    assert M.fec_max_info_bits(16384, F.R12) == 8186


def test_helper_errors():
    L = M.lib()
    n = C.c_size_t(12345)
    for fn in (L.ofdm_fec_coded_bits, L.ofdm_fec_max_info_bits):
        assert fn(100, 0, None) == -1
        assert fn(100, 3, C.byref(n)) == -1 and fn(100, -1, C.byref(n)) == -1
    assert L.ofdm_fec_coded_bits(0, 0, C.byref(n)) == -1
    for rate in F.RATES:
        short = F.coded_bits(1, rate) - 1
        assert L.ofdm_fec_max_info_bits(short, rate, C.byref(n)) == -1
        assert L.ofdm_fec_max_info_bits(0, rate, C.byref(n)) == -1
        assert L.ofdm_fec_max_info_bits(short + 1, rate, C.byref(n)) == 0 and n.value == 1
    with pytest.raises(M.OfdmError) as e:
        M.fec_max_info_bits(3, F.R12)
    assert e.value.code == -1
    n.value = 12345
    assert L.ofdm_fec_coded_bits(0, 0, C.byref(n)) == -1 and n.value == 12345  # untouched on error


def test_workspace_size():
    L = M.lib()
    n = C.c_size_t()
    assert L.ofdm_fec_workspace_size(4, 100, None) == -1
    assert L.ofdm_fec_workspace_size(4, 0, C.byref(n)) == -1
    assert L.ofdm_fec_workspace_size(4, (1 << 20) + 1, C.byref(n)) == -1
    assert L.ofdm_fec_workspace_size(4, 1 << 20, C.byref(n)) == 0
    assert n.value >= 4 * ((1 << 20) + 6) * 8  # one 64-bit survivor word per step
    for nb in (1, 250, 8186):
        w = M.fec_workspace_size(3, nb)
        assert w == 0 or w >= 3 * (nb + 6) * 8
        assert w % 16 == 0
    assert M.fec_workspace_size(0, 8186) == 0
