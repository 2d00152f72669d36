"""Interleaver / scrambler surface of the C ABI that needs no GPU: the exported
symbols and their Python view, and the error returns the host can reach
without a context (a context needs a device: ofdm_interleave_default's values
per config and the errors behind the context check are in
test_gpu_interleave.py)."""
import ctypes as C
import re

import interleave_model as IM
import ofdm_mi355x as M
from common import ALL_CONFIGS

NEW = ("ofdm_interleave_default", "ofdm_interleave_bits", "ofdm_interleave_llr", "ofdm_scramble")


def test_library_exports_the_interleaver_and_the_scrambler():
    L = M.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in M.SIGNATURES
    assert (M.IL_FORWARD, M.IL_INVERSE) == (0, 1)
    for name in ("interleave_default", "interleave_bits", "interleave_llr", "scramble"):
        assert hasattr(M.Modem, name)
    assert L.ofdm_abi_version() == 5


def test_header_declares_what_the_binding_binds():
    with open(M.HEADER) as f:
        h = f.read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
    assert re.search(r"OFDM_IL_FORWARD\s*=\s*0\s*,\s*OFDM_IL_INVERSE\s*=\s*1", h)
    counts = {"ofdm_interleave_default": 4, "ofdm_interleave_bits": 9, "ofdm_interleave_llr": 10, "ofdm_scramble": 10}
    for name, nargs in counts.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", h).group(1)
        assert len(decl.split(",")) == nargs == len(M.SIGNATURES[name][1]), name


def test_default_block_of_every_config_is_valid():
    """What ofdm_interleave_default computes (D*k, 16, max(k/2, 1)) is a valid
    block on all 16 test configs."""
    assert len(ALL_CONFIGS) == 16
    for name, p in ALL_CONFIGS.items():
        k = p["mod_type"]
        assert IM.valid(p["num_data_subc"] * k, 16, max(k // 2, 1)), name


def test_calls_without_a_context_are_invalid_and_launch_nothing():
    """No device exists here: a call that got past its argument checks would
    fail with OFDM_ERR_HIP (-3), not OFDM_ERR_INVALID (-1)."""
    L = M.lib()
    n, c, s = C.c_size_t(777), C.c_size_t(777), C.c_size_t(777)
    buf = (C.c_uint8 * 4096)()
    a, b = C.addressof(buf), C.addressof(buf) + 2048
    assert L.ofdm_interleave_default(None, C.byref(n), C.byref(c), C.byref(s)) == -1
    assert (n.value, c.value, s.value) == (777, 777, 777)  # untouched on error
    assert L.ofdm_interleave_bits(None, a, 1, 48, 16, 1, 0, b, None) == -1
    assert L.ofdm_interleave_llr(None, a, M.LLR_I8, 1, 48, 16, 1, 1, b, None) == -1
    assert L.ofdm_interleave_llr(None, a, 7, 1, 48, 16, 1, 1, b, None) == -1
    assert L.ofdm_scramble(None, a, 6, 1, 48, 127, None, b, 6, None) == -1
    assert b"null" in L.ofdm_last_error()
    assert L.ofdm_interleave_bits(None, a, 0, 48, 16, 1, 0, b, None) == -1  # the context is checked before nblocks
    assert not any(buf)
