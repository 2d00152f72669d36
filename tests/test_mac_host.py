"""MAC framing surface of the C ABI that needs no GPU: the exported symbols,
their Python view and the header's declarations, ofdm_mac_payload_len, and
every OFDM_ERR_INVALID rule of the two batched calls. Those rules are checked
before the context is, so a call without a context (no device exists here)
reaches each of them: its message names the rule, and a call that passes all
of them fails on the null context ("null context") last, still before any
device call (which would return OFDM_ERR_HIP, -3)."""
import ctypes as C
import re

import numpy as np

import ofdm_mi355x as M

NEW = {"ofdm_mac_payload_len": 3, "ofdm_mac_write": 14, "ofdm_mac_read": 12}


def test_library_exports_the_mac_entry_points():
    L = M.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in M.SIGNATURES
    for name in ("mac_write", "mac_read", "mac_payload_len"):
        assert hasattr(M.Modem, name)
    assert (M.FCS_NONE, M.FCS_CRC32) == (0, 1)
    assert L.ofdm_abi_version() == 5  # additive: the ABI version stays


def test_header_declares_what_the_binding_binds():
    with open(M.HEADER) as f:
        h = f.read()
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", h).group(1)
        assert len(decl.split(",")) == nargs == len(M.SIGNATURES[name][1]), name
    assert re.search(r"OFDM_FCS_NONE\s*=\s*0\s*,\s*OFDM_FCS_CRC32\s*=\s*1", h)
    lead = h[:h.index("#ifndef OFDM_MI355X_H")]
    assert "mac_write" in lead and "mac_read" in lead, "missing from the capturable list"
    assert "#define OFDM_MI355X_ABI_VERSION 5" in h


def test_info_dtype_is_the_headers_struct():
    dt = M.mac_info_dtype()
    assert dt.itemsize == 16
    assert [dt.fields[n][1] for n in ("tx_id", "rx_id", "seq_num", "cs", "cs_calc", "cs_ok", "fcs_ok", "ok",
                                      "reserved")] == [0, 2, 4, 6, 8, 10, 11, 12, 13]


def test_payload_len_values_and_errors():
    L = M.lib()
    assert M.mac_payload_len(256, M.FCS_NONE) == 248
    assert M.mac_payload_len(256, M.FCS_CRC32) == 244
    assert M.mac_payload_len(8, M.FCS_NONE) == 0
    assert M.mac_payload_len(12, M.FCS_CRC32) == 0
    assert M.mac_payload_len(65536, M.FCS_CRC32) == 65524
    cap = C.c_size_t(777)
    for frame_len, fcs in ((7, 0), (11, 1), (65537, 0), (65537, 1), (0, 0), (256, 2), (256, -1)):
        assert L.ofdm_mac_payload_len(frame_len, fcs, C.byref(cap)) == -1, (frame_len, fcs)
        assert cap.value == 777  # untouched on error
    assert L.ofdm_mac_payload_len(256, 0, None) == -1


def _bufs():
    buf = np.zeros(8192 + 64, np.uint8)
    a = (buf.ctypes.data + 15) & ~15
    return buf, a, a + 4096


def test_write_rules_return_invalid_without_a_context():
    L = M.lib()
    buf, a, b = _bufs()

    def wr(payload=a, pstride=244, plen=244, nframes=2, frame_len=256, fcs=1, tx=1, rx=0, seq0=0, seqs=None, out=b,
           fstride=256):
        rc = L.ofdm_mac_write(None, payload, pstride, plen, nframes, frame_len, fcs, tx, rx, seq0, seqs, out, fstride,
                              None)
        return rc, L.ofdm_last_error().decode()

    assert wr() == (-1, "null context")  # every rule passes: the context is what is missing
    assert wr(nframes=0) == (-1, "null context")  # the context is checked before nframes == 0 returns
    cases = [
        (dict(fcs=2), "fcs"), (dict(fcs=-1), "fcs"),
        (dict(frame_len=11, plen=0, pstride=0), "frame_len"), (dict(frame_len=7, fcs=0, plen=0), "frame_len"),
        (dict(frame_len=65537, fstride=65537), "frame_len"),
        (dict(plen=245, pstride=245), "payload_len"), (dict(fcs=0, plen=249, pstride=249), "payload_len"),
        (dict(pstride=243), "payload_stride"), (dict(fstride=255), "frame_stride"),
        (dict(tx=65536), "16-bit"), (dict(rx=65536), "16-bit"), (dict(seq0=65536), "16-bit"),
        (dict(seqs=a + 1), "seqs"),
        (dict(out=None), "null argument"), (dict(payload=None), "null argument"),
        (dict(out=a + 100), "overlap"), (dict(payload=b + 500), "overlap"), (dict(out=a), "overlap"),
        (dict(nframes=2 ** 62), "nframes"),
    ]
    for kw, word in cases:
        rc, msg = wr(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert wr(payload=None, plen=0, pstride=0) == (-1, "null context")  # no payload bytes: no payload pointer needed
    assert wr(frame_len=12, plen=0, pstride=0, fstride=12)[0] == -1
    assert not buf.any()


def test_read_rules_return_invalid_without_a_context():
    L = M.lib()
    buf, a, b = _bufs()
    info, errs = b + 1024, b + 2048

    def rd(frames=a, fstride=256, nframes=2, frame_len=256, fcs=1, expect=-1, out=b, pstride=244, info=info, errs=errs):
        rc = L.ofdm_mac_read(None, frames, fstride, nframes, frame_len, fcs, expect, out, pstride, info, errs, None)
        return rc, L.ofdm_last_error().decode()

    assert rd() == (-1, "null context")
    assert rd(nframes=0) == (-1, "null context")
    for alone in (dict(info=None, errs=None), dict(out=None, errs=None), dict(out=None, info=None)):
        assert rd(**alone) == (-1, "null context")  # one output is enough: only the context is missing
    cases = [
        (dict(fcs=3), "fcs"), (dict(frame_len=11), "frame_len"), (dict(frame_len=65537, fstride=65537), "frame_len"),
        (dict(fstride=255), "frame_stride"), (dict(pstride=243), "payload_stride"),
        (dict(fcs=0, pstride=247), "payload_stride"), (dict(expect=65536), "expect_rx_id"),
        (dict(info=info + 8), "info_out"), (dict(errs=errs + 4), "frame_errors"),
        (dict(out=a + 16), "overlap"), (dict(info=a + 256), "overlap"), (dict(errs=a + 8), "overlap"),
        (dict(nframes=2 ** 62), "nframes"),
    ]
    for kw, word in cases:
        rc, msg = rd(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert rd(frames=None) == (-1, "null argument")
    assert rd(out=None, info=None, errs=None) == (-1, "null argument")
    assert rd(out=None, pstride=0) == (-1, "null context")  # the stride of an absent payload_out is not looked at
    assert not buf.any()
