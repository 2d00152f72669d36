"""ofdm_mac_write / ofdm_mac_read on the GPU against tests/mac_model.py: every
comparison is bit for bit. Output buffers are filled with a sentinel first, so
the bytes a call must not write (past frame_stride * nframes, between a
payload's capacity and its stride, past the end) are checked too."""
import functools
import zlib

import numpy as np
import pytest

import fec_model as F
import interleave_model as IM
import mac_model as MM
import oracle as O
import soft_model as SM
from common import EXTRA, golden
from test_gpu_graph import replay_protocol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

SENTINEL = 0xA5
PAD = 64
INFO = M.mac_info_dtype()


@functools.lru_cache(maxsize=None)
def modem():
    return M.Modem(EXTRA["N128_k4_s3"], 0)


def dev_at(nbytes, mis=0, fill=SENTINEL):
    """A sentinel-filled tensor of nbytes + PAD bytes whose address is `mis` past a 16-byte boundary."""
    base = torch.full((nbytes + PAD + 32,), fill, dtype=torch.uint8, device="cuda")
    off = (-base.data_ptr()) % 16 + mis
    t = base[off:off + nbytes + PAD]
    assert t.data_ptr() % 16 == mis % 16
    return t


def upload(a, mis=0):
    a = np.array(a, np.uint8).reshape(-1)  # (a copy: torch wants a writable array)
    t = dev_at(a.size, mis)
    t[:a.size].copy_(torch.from_numpy(a))
    return t


def strided(rows, stride, fill=0):
    """(nframes, len) rows laid out stride bytes apart (the last one ends at its length)."""
    n, ln = rows.shape
    out = np.full((n - 1) * stride + ln, fill, np.uint8)
    for f in range(n):
        out[f * stride:f * stride + ln] = rows[f]
    return out


def model_frames(payloads, tx, rx, seqs, frame_len, fcs):
    return np.stack([MM.write(payloads[f], tx, rx, int(seqs[f]), frame_len, fcs) for f in range(len(payloads))])


def model_infos(frames, fcs, expect=-1):
    out = np.zeros(len(frames), INFO)
    for f, fr in enumerate(frames):
        for k, v in MM.read(fr, fcs, expect)[1].items():
            out[k][f] = v
    return out


def info_buf(nframes):
    return dev_at(nframes * 16, 0)


def infos(t, nframes):
    return t[:nframes * 16].cpu().numpy().view(INFO)


def counter():
    return torch.zeros((1,), dtype=torch.int64, device="cuda")


def test_golden_frame():
    g = golden()
    m = modem()
    pl = upload(g["payload_text"])
    out = dev_at(256)
    m.mac_write(pl, 248, 1, 256, out, fcs=M.FCS_NONE, tx_id=1, rx_id=0, seq0=0)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert h[:256].tobytes() == g["payload"].tobytes()
    assert np.all(h[256:] == SENTINEL)
    back, info, errs = dev_at(248), info_buf(1), counter()
    m.mac_read(out, 1, 256, fcs=M.FCS_NONE, payload_out=back, info_out=info, frame_errors=errs)
    torch.cuda.synchronize()
    hb = back.cpu().numpy()
    assert hb[:248].tobytes() == g["payload_text"].tobytes() and np.all(hb[248:] == SENTINEL)
    i = infos(info, 1)[0]
    assert (i["tx_id"], i["rx_id"], i["seq_num"], i["cs"], i["cs_calc"]) == (1, 0, 0, 0x577E, 0x577E)
    assert (i["cs_ok"], i["fcs_ok"], i["ok"]) == (1, 1, 1) and not i["reserved"].any()
    assert int(errs.item()) == 0


def _length_cases():
    """8 + F, 9 + F and the issue's lengths from 15 on, none below 8 + F."""
    cases = []
    for fcs, f4 in ((M.FCS_NONE, 0), (M.FCS_CRC32, 4)):
        lens = {8 + f4, 9 + f4, 15, 16, 17, 63, 64, 65, 255, 1023, 1024, 1025, 4096, 4099, 65536}
        cases += [(n, fcs) for n in sorted(lens) if n >= 8 + f4]
    return cases


@pytest.mark.parametrize("frame_len,fcs", _length_cases())
def test_lengths_strides_and_alignments(frame_len, fcs):
    """5 frames (more than the 4 waves of a workgroup) at the lengths where the
    wave tiling changes: a chunk, a row of 64 chunks, both chunk widths.
    Payloads of 0, 1, cap - 1 and cap bytes; strides of the length and of the
    length + 3 (frames at every alignment: the byte path, and the wide path
    where the length + 3 is a multiple of 4); buffers at a 16-byte boundary
    and one byte past it."""
    m, nf = modem(), 5
    cap = M.mac_payload_len(frame_len, fcs)
    assert cap == MM.payload_len(frame_len, fcs)
    rng = np.random.default_rng(frame_len * 2 + fcs)
    seqs = [65534, 65535, 0, 1, 2]
    for plen in sorted({0, 1, max(cap - 1, 0), cap} & set(range(cap + 1))):
        payloads = rng.integers(0, 256, (nf, plen), dtype=np.uint8)
        frames = model_frames(payloads, 0xBEEF, 0x1234, seqs, frame_len, fcs)
        want_info = model_infos(frames, fcs)
        assert want_info["ok"].all()
        for extra in (0, 3):
            for mis in (0, 1):
                what = (frame_len, fcs, plen, extra, mis)
                fstride, pstride, ostride = frame_len + extra, plen + extra, cap + extra
                d_pl = upload(strided(payloads, pstride) if plen else np.zeros(1, np.uint8), mis)
                d_fr = dev_at(nf * fstride, mis)
                m.mac_write(d_pl, plen, nf, frame_len, d_fr, fcs=fcs, tx_id=0xBEEF, rx_id=0x1234, seq0=65534,
                            payload_stride=pstride, frame_stride=fstride)
                torch.cuda.synchronize()
                h = d_fr.cpu().numpy()
                got = h[:nf * fstride].reshape(nf, fstride)
                assert np.array_equal(got[:, :frame_len], frames), what
                assert not got[:, frame_len:].any(), ("bytes up to the stride must be zeros", what)
                assert np.all(h[nf * fstride:] == SENTINEL), what

                d_in = upload(strided(frames, fstride, fill=0x3C), mis)
                d_out = dev_at(nf * ostride, mis)
                d_info, errs = info_buf(nf), counter()
                m.mac_read(d_in, nf, frame_len, fcs=fcs, payload_out=d_out, info_out=d_info, frame_errors=errs,
                           frame_stride=fstride, payload_stride=ostride)
                torch.cuda.synchronize()
                ho = d_out.cpu().numpy()
                rows = ho[:nf * ostride].reshape(nf, ostride)
                assert np.array_equal(rows[:, :cap], frames[:, 8:8 + cap]), what
                assert np.all(rows[:, cap:] == SENTINEL) and np.all(ho[nf * ostride:] == SENTINEL), what
                assert np.array_equal(infos(d_info, nf), want_info), what
                assert np.all(d_info.cpu().numpy()[nf * 16:] == SENTINEL)
                assert int(errs.item()) == 0
                assert np.array_equal(d_in.cpu().numpy()[:(nf - 1) * fstride + frame_len],
                                      strided(frames, fstride, fill=0x3C)), "the input is not modified"


def test_sequence_numbers_and_ids():
    m, nf, frame_len = modem(), 5, 64
    pl = np.random.default_rng(3).integers(0, 256, (nf, 52), dtype=np.uint8)
    d_pl, d_fr = upload(pl), dev_at(nf * frame_len)
    m.mac_write(d_pl, 52, nf, frame_len, d_fr, tx_id=0, rx_id=65535, seq0=65534)
    torch.cuda.synchronize()
    got = d_fr.cpu().numpy()[:nf * frame_len].reshape(nf, frame_len)
    assert got[:, 4:6].copy().view("<u2").reshape(-1).tolist() == [65534, 65535, 0, 1, 2]
    assert np.array_equal(got, model_frames(pl, 0, 65535, [65534, 65535, 0, 1, 2], frame_len, M.FCS_CRC32))
    seqs = np.array([7, 65535, 0, 300, 7], np.uint16)
    d_seqs = torch.from_numpy(seqs.view(np.int16)).cuda()
    m.mac_write(d_pl, 52, nf, frame_len, d_fr, tx_id=65535, rx_id=0, seq0=9, seqs=d_seqs)
    torch.cuda.synchronize()
    got = d_fr.cpu().numpy()[:nf * frame_len].reshape(nf, frame_len)
    assert np.array_equal(got, model_frames(pl, 65535, 0, seqs, frame_len, M.FCS_CRC32))
    d_info = info_buf(nf)
    m.mac_read(d_fr, nf, frame_len, info_out=d_info, expect_rx_id=0)
    torch.cuda.synchronize()
    i = infos(d_info, nf)
    assert i["seq_num"].tolist() == seqs.tolist() and i["ok"].all()
    assert (i["tx_id"] == 65535).all() and (i["rx_id"] == 0).all()


def test_detection():
    """64 frames of 1023 bytes with a CRC-32. One flipped bit per frame, at
    positions spread over header, cs, payload and FCS: every frame fails. Two
    unequal payload bytes swapped: the sum still holds, the CRC does not.
    Untouched frames add nothing to frame_errors; the counter accumulates."""
    m, nf, frame_len = modem(), 64, 1023
    cap = MM.payload_len(frame_len, MM.FCS_CRC32)
    rng = np.random.default_rng(11)
    pl = rng.integers(0, 256, (nf, cap), dtype=np.uint8)
    frames = model_frames(pl, 5, 6, np.arange(nf), frame_len, MM.FCS_CRC32)
    d_info, errs = info_buf(nf), counter()

    def read(fr, expect=-1):
        m.mac_read(upload(fr), nf, frame_len, info_out=d_info, frame_errors=errs, expect_rx_id=expect)
        torch.cuda.synchronize()
        return infos(d_info, nf).copy()

    errs.fill_(1000)
    i = read(frames)
    assert i["ok"].all() and int(errs.item()) == 1000, "good frames must leave the counter as it is"

    flipped = frames.copy()
    pos = np.concatenate([np.arange(8), [1019, 1020, 1021, 1022], np.linspace(8, 1018, nf - 12).astype(int)])
    assert len(pos) == nf and {0, 6, 7, 8, 1018, 1019, 1022} <= set(pos.tolist())
    for f in range(nf):
        flipped[f, pos[f]] ^= 1 << (f % 8)
    i = read(flipped)
    assert np.array_equal(i, model_infos(flipped, MM.FCS_CRC32))
    assert not i["ok"].any() and int(errs.item()) == 1000 + nf
    assert not i["fcs_ok"].any(), "a single flipped bit anywhere breaks the CRC"

    swapped = frames.copy()
    for f in range(nf):
        a = 8 + f
        b = a + 1 + int(np.argmax(swapped[f, a + 1:8 + cap] != swapped[f, a]))
        assert swapped[f, a] != swapped[f, b]
        swapped[f, [a, b]] = swapped[f, [b, a]]
    i = read(swapped)
    assert i["cs_ok"].all() and not i["fcs_ok"].any() and not i["ok"].any()
    assert int(errs.item()) == 1000 + 2 * nf, "frame_errors accumulates over launches"

    i = read(frames, expect=7)
    assert i["cs_ok"].all() and i["fcs_ok"].all() and not i["ok"].any()
    assert int(errs.item()) == 1000 + 3 * nf
    i = read(frames, expect=6)
    assert i["ok"].all() and int(errs.item()) == 1000 + 3 * nf


@pytest.mark.parametrize("fcs", [M.FCS_NONE, M.FCS_CRC32])
def test_large_batch(fcs):
    """4099 frames of 255 bytes: more frames than the grid has waves and a grid tail."""
    m, nf, frame_len = modem(), 4099, 255
    cap = MM.payload_len(frame_len, fcs)
    rng = np.random.default_rng(17 + fcs)
    pl = rng.integers(0, 256, (nf, cap), dtype=np.uint8)
    seqs = (np.arange(nf) + 60000) % 65536
    frames = model_frames(pl, 9, 10, seqs, frame_len, fcs)
    d_fr = dev_at(nf * frame_len)
    m.mac_write(upload(pl), cap, nf, frame_len, d_fr, fcs=fcs, tx_id=9, rx_id=10, seq0=60000)
    torch.cuda.synchronize()
    h = d_fr.cpu().numpy()
    assert np.array_equal(h[:nf * frame_len].reshape(nf, frame_len), frames) and np.all(h[nf * frame_len:] == SENTINEL)
    # all-random bytes as received frames: the verdicts are the model's (all bad, bar an accident)
    noise = rng.integers(0, 256, (nf, frame_len), dtype=np.uint8)
    noise[::3] = frames[::3]
    d_out, d_info, errs = dev_at(nf * cap), info_buf(nf), counter()
    m.mac_read(upload(noise), nf, frame_len, fcs=fcs, payload_out=d_out, info_out=d_info, frame_errors=errs)
    torch.cuda.synchronize()
    want = model_infos(noise, fcs)
    assert np.array_equal(infos(d_info, nf), want)
    assert int(errs.item()) == int((want["ok"] == 0).sum()) >= nf // 2
    ho = d_out.cpu().numpy()
    assert np.array_equal(ho[:nf * cap].reshape(nf, cap), noise[:, 8:8 + cap]) and np.all(ho[nf * cap:] == SENTINEL)


def test_each_output_alone():
    m, nf, frame_len = modem(), 6, 100
    cap = MM.payload_len(frame_len, MM.FCS_CRC32)
    pl = np.random.default_rng(23).integers(0, 256, (nf, cap), dtype=np.uint8)
    frames = model_frames(pl, 1, 2, np.arange(nf), frame_len, MM.FCS_CRC32)
    frames[4, 50] ^= 8
    d_in = upload(frames)
    d_out, d_info, errs = dev_at(nf * cap), info_buf(nf), counter()
    m.mac_read(d_in, nf, frame_len, payload_out=d_out)
    m.mac_read(d_in, nf, frame_len, info_out=d_info)
    m.mac_read(d_in, nf, frame_len, frame_errors=errs)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy()[:nf * cap].reshape(nf, cap), frames[:, 8:8 + cap])
    assert np.array_equal(infos(d_info, nf), model_infos(frames, MM.FCS_CRC32))
    assert infos(d_info, nf)["ok"].tolist() == [1, 1, 1, 1, 0, 1]
    assert int(errs.item()) == 1


def test_invalid_arguments_behind_the_context_launch_nothing():
    """The rules of tests/test_mac_host.py with a live context: still
    OFDM_ERR_INVALID, nothing written; nframes == 0 is OFDM_OK."""
    m, L = modem(), M.lib()
    src, dst = dev_at(1024, fill=5), dev_at(1024)
    st = torch.cuda.current_stream().cuda_stream
    a, b = src.data_ptr(), dst.data_ptr()
    assert L.ofdm_mac_write(m.h, a, 52, 52, 4, 64, 2, 0, 0, 0, None, b, 64, st) == -1
    assert L.ofdm_mac_write(m.h, a, 52, 53, 4, 64, 1, 0, 0, 0, None, b, 64, st) == -1
    assert L.ofdm_mac_write(m.h, a, 52, 52, 4, 64, 1, 65536, 0, 0, None, b, 64, st) == -1
    assert L.ofdm_mac_write(m.h, a, 52, 52, 4, 64, 1, 0, 0, 0, None, a + 8, 64, st) == -1
    assert L.ofdm_mac_read(m.h, a, 64, 4, 64, 1, -1, None, 0, None, None, st) == -1
    assert L.ofdm_mac_read(m.h, a, 64, 4, 64, 1, -1, None, 0, b + 8, None, st) == -1
    assert L.ofdm_mac_read(m.h, a, 63, 4, 64, 1, -1, b, 52, None, None, st) == -1
    assert L.ofdm_mac_write(m.h, a, 52, 52, 0, 64, 1, 0, 0, 0, None, b, 64, st) == 0
    assert L.ofdm_mac_read(m.h, a, 64, 0, 64, 1, -1, b, 52, None, None, st) == 0
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all()) and bool((src == 5).all()), "an invalid call launched something"


def test_graph_capture_of_write_then_read():
    """test_gpu_graph.py's protocol on mac_write -> mac_read: replay 1 equals
    the eager run, replay 2 on overwritten payloads equals a fresh eager run;
    both equal the model, and frame_errors holds the replays' sum."""
    m, nf, frame_len = modem(), 37, 300
    cap = MM.payload_len(frame_len, MM.FCS_CRC32)
    d_pl = torch.zeros((nf * cap,), dtype=torch.uint8, device="cuda")
    d_fr, d_out, d_info = dev_at(nf * 304), dev_at(nf * cap), info_buf(nf)
    errs = counter()

    def payloads(c):
        return np.random.default_rng(40 + c).integers(0, 256, (nf, cap), dtype=np.uint8)

    def run():
        m.mac_write(d_pl, cap, nf, frame_len, d_fr, tx_id=3, rx_id=4, seq0=65530, frame_stride=304)
        # a second read with another address filter: every frame fails it and is counted
        m.mac_read(d_fr, nf, frame_len, payload_out=d_out, info_out=d_info, frame_errors=errs, expect_rx_id=4,
                   frame_stride=304)
        m.mac_read(d_fr, nf, frame_len, frame_errors=errs, expect_rx_id=5, frame_stride=304)

    outs = {"frames": d_fr, "payload": d_out, "info": d_info}
    live = {"frames": nf * 304, "payload": nf * cap, "info": nf * 16}
    _, _, r1, r2, counts = replay_protocol(run, lambda c: d_pl.copy_(torch.from_numpy(payloads(c).reshape(-1))), outs,
                                           live, counters=[errs])
    for c, r in ((0, r1), (1, r2)):
        frames = model_frames(payloads(c), 3, 4, (65530 + np.arange(nf)) % 65536, frame_len, MM.FCS_CRC32)
        got = r["frames"][:nf * 304].reshape(nf, 304)
        assert np.array_equal(got[:, :frame_len], frames) and not got[:, frame_len:].any()
        assert np.array_equal(r["payload"][:nf * cap].reshape(nf, cap), payloads(c))
        assert np.array_equal(r["info"][:nf * 16].view(INFO), model_infos(frames, MM.FCS_CRC32, 4))
    assert counts == [2 * nf]


# ------------------------------------------------------------------ end to end
E2E_REL_NOISE, E2E_SEED, E2E_SCALE = 0.4, 9, 8.0


@functools.lru_cache(maxsize=None)
def e2e_cpu():
    """The coded link of test_coded_link_end_to_end in numpy (oracle tx, awgn
    and rx points; the soft, interleaver, Viterbi and MAC models)."""
    p = EXTRA["N128_k4_s3"]
    g, k, D = O.geometry(p), p["mod_type"], p["num_data_subc"]
    nf, cap_bits = 32, g["bytes_per_frame"] * 8
    nb = F.max_info_bits(cap_bits, F.R12)
    frame_len, nbytes = nb // 8, (nb + 7) // 8
    pl = np.random.default_rng(31).integers(0, 256, (nf, MM.payload_len(frame_len, MM.FCS_CRC32)), dtype=np.uint8)
    seqs = (65520 + np.arange(nf)) % 65536
    frames = np.zeros((nf, nbytes), np.uint8)
    frames[:, :frame_len] = model_frames(pl, 3, 4, seqs, frame_len, MM.FCS_CRC32)
    seeds = (np.arange(nf) * 37 % 256).astype(np.uint8)
    coded = F.encode(IM.scramble(F.unpack(frames, nb), seeds), F.R12)
    frame = np.zeros((nf, cap_bits), np.uint8)
    frame[:, :coded.shape[1]] = coded
    n, c, s = D * k, 16, max(k // 2, 1)
    sent = F.pack(IM.interleave(frame, n, c, s))
    x = O.tx_batch(p, sent.reshape(-1), nf)
    rms = float(np.sqrt(np.mean(np.abs(x) ** 2)))
    iq = O.awgn(x, rms * E2E_REL_NOISE, seed=E2E_SEED)
    E, _, _ = O.rx_batch(p, iq, nf, g["message_len"])
    L = np.clip(np.rint(SM.ref_llr(k, E.reshape(nf, -1), E2E_SCALE)), -127, 127).astype(np.int64)
    dec, _ = F.viterbi(IM.deinterleave(L.reshape(nf, -1), n, c, s).reshape(nf, -1), nb, F.R12)
    out = F.pack(IM.scramble(dec, seeds))
    lost = int(np.any(out[:, :frame_len] != frames[:, :frame_len], axis=1).sum())
    return dict(p=p, g=g, nf=nf, nb=nb, frame_len=frame_len, nbytes=nbytes, pl=pl, frames=frames, seeds=seeds,
                sent=sent, rms=rms, model_lost=lost)


def test_coded_link_end_to_end():
    """N128_k4_s3, rate 1/2, 32 frames, one codeword per frame: mac_write
    (frame_len = floor(378 / 8) = 47, CRC-32, frame_stride 48) -> scramble ->
    fec_encode -> interleave -> tx with AWGN -> rx_soft (int8, scale 8) ->
    deinterleave -> fec_decode -> scramble -> mac_read. info.ok is 0 exactly
    for the frames whose decoded bytes differ from the sent ones, and
    frame_errors is their count. Noise std 0.4 of the tx samples' rms, seed 9
    (chosen on the CPU with e2e_cpu, the numpy chain: it loses 8 of the 32
    codewords there; 0.35 loses 3, 0.45 loses 19, 0.3 none, 0.5 29)."""
    c = e2e_cpu()
    assert 2 <= c["model_lost"] <= 30
    p, g, nf, nb, frame_len, nbytes = c["p"], c["g"], c["nf"], c["nb"], c["frame_len"], c["nbytes"]
    m, k, S = modem(), p["mod_type"], p["num_symb"]
    u8, cap_bits, nsym = torch.uint8, g["bytes_per_frame"] * 8, nf * S
    seeds = torch.from_numpy(c["seeds"]).cuda()
    d_frames, d_scr = dev_at(nf * nbytes), torch.empty((nf * nbytes,), dtype=u8, device="cuda")
    coded = torch.empty((nf * g["bytes_per_frame"],), dtype=u8, device="cuda")
    sent = torch.empty_like(coded)
    iq = torch.empty((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
    llr = torch.empty((nf * cap_bits,), dtype=torch.int8, device="cuda")
    dellr = torch.empty_like(llr)
    dec, out = torch.empty_like(d_scr), torch.empty_like(d_scr)
    d_pay, d_info, errs = dev_at(nf * c["pl"].shape[1]), info_buf(nf), counter()
    wsz = M.fec_workspace_size(nf, nb)
    ws = torch.empty((wsz,), dtype=u8, device="cuda") if wsz else None

    m.mac_write(upload(c["pl"]), c["pl"].shape[1], nf, frame_len, d_frames, tx_id=3, rx_id=4, seq0=65520,
                frame_stride=nbytes)
    m.scramble(d_frames, nf, nb, d_scr, seeds=seeds)
    m.fec_encode(d_scr, nf, nb, F.R12, coded, coded_stride=g["bytes_per_frame"])
    m.interleave_bits(coded, nsym, sent, M.IL_FORWARD)
    m.tx(sent, nf, iq, noise_std=c["rms"] * E2E_REL_NOISE, seed=E2E_SEED)
    m.rx_soft(iq, nf, llr, E2E_SCALE, M.LLR_I8)
    m.interleave_llr(llr, nsym, dellr, M.IL_INVERSE, fmt=M.LLR_I8)
    m.fec_decode(dellr, nf, nb, F.R12, dec, fmt=M.LLR_I8, llr_stride=cap_bits, workspace=ws)
    m.scramble(dec, nf, nb, out, seeds=seeds)
    m.mac_read(out, nf, frame_len, payload_out=d_pay, info_out=d_info, frame_errors=errs, expect_rx_id=4,
               frame_stride=nbytes)
    torch.cuda.synchronize()

    assert np.array_equal(d_frames.cpu().numpy()[:nf * nbytes].reshape(nf, nbytes), c["frames"])
    assert np.array_equal(sent.cpu().numpy().reshape(nf, -1), c["sent"])
    got = out.cpu().numpy().reshape(nf, nbytes)
    lost = np.any(got[:, :frame_len] != c["frames"][:, :frame_len], axis=1)
    print("codewords lost on the GPU:", int(lost.sum()), "in the numpy chain:", c["model_lost"])
    assert 1 <= int(lost.sum()) <= nf - 1, "the link must lose some codewords and keep some"
    i = infos(d_info, nf)
    assert np.array_equal(i["ok"] == 0, lost)
    assert int(errs.item()) == int(lost.sum())
    assert np.array_equal(i, model_infos(got[:, :frame_len], MM.FCS_CRC32, 4))
    pay = d_pay.cpu().numpy()[:nf * c["pl"].shape[1]].reshape(nf, -1)
    assert np.array_equal(pay[~lost], c["pl"][~lost])
    assert zlib.crc32(c["frames"][0, :frame_len].tobytes()) == MM.RESIDUE
