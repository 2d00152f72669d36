"""The frequency-selective channel surface of the C ABI that needs no GPU: the
exported symbols, their Python view and the header's declarations, and the
error returns the host can reach without a context (the errors behind the
context check are in test_gpu_csi.py)."""
import ctypes as C
import re

import ofdm_mi355x as M

NEW = {"ofdm_chan_estimate_ls": 10, "ofdm_soft_demap_csi": 10}


def test_library_exports_both_entry_points():
    L = M.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in M.SIGNATURES
    for name in ("chan_estimate_ls", "soft_demap_csi"):
        assert hasattr(M.Modem, name)
    assert L.ofdm_abi_version() == 5  # additive: the ABI version stays


def test_header_declares_what_the_binding_binds():
    with open(M.HEADER) as f:
        h = f.read()
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", h).group(1)
        assert len(decl.split(",")) == nargs == len(M.SIGNATURES[name][1]), name
    lead = h[:h.index("#ifndef OFDM_MI355X_H")]
    assert "chan_estimate_ls" in lead and "soft_demap_csi" in lead, "missing from the capturable list"
    assert "per-carrier weighting of the LLRs" not in h


def test_calls_without_a_context_are_invalid_and_launch_nothing():
    """No device exists here: a call that got past its argument checks would
    fail with OFDM_ERR_HIP (-3), not OFDM_ERR_INVALID (-1)."""
    L = M.lib()
    buf = (C.c_uint8 * 4096)()
    a, b = C.addressof(buf), C.addressof(buf) + 2048
    assert L.ofdm_chan_estimate_ls(None, a, 1, 64, 0, b, 64, None, 64, None) == -1
    assert b"null" in L.ofdm_last_error()
    assert L.ofdm_soft_demap_csi(None, a, 1, a, 0, 1.0, None, M.LLR_F32, b, None) == -1
    assert L.ofdm_chan_estimate_ls(None, a, 0, 64, 0, b, 64, None, 64, None) == -1  # the context is checked first
    assert L.ofdm_soft_demap_csi(None, a, 0, a, 0, 1.0, None, M.LLR_I8, b, None) == -1
    assert not any(buf)
