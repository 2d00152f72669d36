"""numpy model of the MAC framing of include/ofdm_mi355x.h ("MAC framing and
frame check"): the reference's 8-byte header {tx_id, rx_id, seq_num, cs}
(little-endian uint16), the payload zero-filled to the frame's capacity, and
with FCS_CRC32 zlib's CRC-32 of everything before it, little-endian."""
import zlib

import numpy as np

FCS_NONE, FCS_CRC32 = 0, 1
HDR = 8
RESIDUE = 0x2144DF1C  # zlib.crc32 of a good frame, FCS included


def payload_len(frame_len, fcs):
    return frame_len - HDR - (4 if fcs == FCS_CRC32 else 0)


def checksum(frame, fcs):
    """MAC::calc_cs: sum of the covered bytes without 6 and 7, mod 2^16."""
    m = len(frame) - (4 if fcs == FCS_CRC32 else 0)
    return (int(frame[:m].sum(dtype=np.int64)) - int(frame[6]) - int(frame[7])) & 0xffff


def write(payload, tx, rx, seq, frame_len, fcs):
    f = 4 if fcs == FCS_CRC32 else 0
    payload = np.asarray(payload, np.uint8)
    assert frame_len >= HDR + f and len(payload) <= frame_len - HDR - f
    frame = np.zeros(frame_len, np.uint8)
    frame[:6] = np.array([tx, rx, seq], "<u2").view(np.uint8)
    frame[HDR:HDR + len(payload)] = payload
    frame[6:8] = np.array([checksum(frame, fcs)], "<u2").view(np.uint8)
    if f:
        frame[-4:] = np.array([zlib.crc32(frame[:-4].tobytes())], "<u4").view(np.uint8)
    return frame


def read(frame, fcs, expect_rx_id=-1):
    """(payload, info): info has the fields of ofdm_mac_info."""
    frame = np.asarray(frame, np.uint8)
    f = 4 if fcs == FCS_CRC32 else 0
    tx, rx, seq, cs = (int(v) for v in frame[:8].view("<u2"))
    calc = checksum(frame, fcs)
    fcs_ok = int(not f or zlib.crc32(frame[:-4].tobytes()) == int(frame[-4:].view("<u4")[0]))
    ok = int(cs == calc and fcs_ok and (expect_rx_id < 0 or rx == expect_rx_id))
    info = dict(tx_id=tx, rx_id=rx, seq_num=seq, cs=cs, cs_calc=calc, cs_ok=int(cs == calc), fcs_ok=fcs_ok, ok=ok)
    return frame[HDR:len(frame) - f].copy(), info
