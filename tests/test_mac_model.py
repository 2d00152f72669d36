"""The numpy MAC model against the committed golden frame and zlib."""
import zlib

import numpy as np

import mac_model as MM
from common import golden


def test_fcs_none_frame_is_the_golden_frame():
    g = golden()
    frame = MM.write(g["payload_text"], tx=1, rx=0, seq=0, frame_len=256, fcs=MM.FCS_NONE)
    assert frame.tobytes() == g["payload"].tobytes()
    assert frame[:8].tolist() == [0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x7E, 0x57]
    assert MM.checksum(frame, MM.FCS_NONE) == 0x577E
    pl, info = MM.read(frame, MM.FCS_NONE)
    assert pl.tobytes() == g["payload_text"].tobytes()
    assert info == dict(tx_id=1, rx_id=0, seq_num=0, cs=0x577E, cs_calc=0x577E, cs_ok=1, fcs_ok=1, ok=1)


def test_crc32_frame_ends_in_zlibs_crc_and_has_the_residue():
    g = golden()
    for pl in (g["payload_text"], g["payload_text"][:100], np.zeros(0, np.uint8)):
        frame = MM.write(pl, tx=1, rx=0, seq=0, frame_len=260, fcs=MM.FCS_CRC32)
        assert int(frame[-4:].view("<u4")[0]) == zlib.crc32(frame[:-4].tobytes())
        assert zlib.crc32(frame.tobytes()) == 0x2144DF1C == MM.RESIDUE
        assert MM.checksum(frame, MM.FCS_CRC32) == int(frame[6:8].view("<u2")[0])
        assert MM.read(frame, MM.FCS_CRC32)[1]["ok"] == 1
    # the same payload in 260 bytes with a CRC: header and payload bytes are the golden frame's
    frame = MM.write(g["payload_text"], 1, 0, 0, 260, MM.FCS_CRC32)
    assert frame[:256].tobytes() == g["payload"].tobytes()


def test_read_tells_sum_from_crc_and_filters_rx_id():
    rng = np.random.default_rng(5)
    frame = MM.write(rng.integers(0, 256, 100, dtype=np.uint8), 7, 9, 65535, 128, MM.FCS_CRC32)
    assert MM.payload_len(128, MM.FCS_CRC32) == 116 and MM.payload_len(128, MM.FCS_NONE) == 120
    assert MM.read(frame, MM.FCS_CRC32, expect_rx_id=9)[1]["ok"] == 1
    info = MM.read(frame, MM.FCS_CRC32, expect_rx_id=8)[1]
    assert (info["cs_ok"], info["fcs_ok"], info["ok"]) == (1, 1, 0)
    swapped = frame.copy()
    assert swapped[10] != swapped[20]
    swapped[[10, 20]] = swapped[[20, 10]]
    info = MM.read(swapped, MM.FCS_CRC32)[1]
    assert (info["cs_ok"], info["fcs_ok"], info["ok"]) == (1, 0, 0)
    flipped = frame.copy()
    flipped[50] ^= 4
    info = MM.read(flipped, MM.FCS_CRC32)[1]
    assert (info["cs_ok"], info["fcs_ok"], info["ok"]) == (0, 0, 0)
