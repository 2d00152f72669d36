"""Channel code on the GPU: ofdm_fec_encode and ofdm_fec_decode against the
numpy model of tests/fec_model.py (bit for bit where the input is integer
valued; by path metric for real-valued float LLRs), the counters, stream
order, every error return, and a small coded link end to end.

Every output buffer carries sentinels past (and, with stride slack, between)
the bytes a launch may write; every input is checked unmodified."""
import ctypes as C
import functools

import numpy as np
import pytest

import fec_model as F
import oracle as O
import soft_model as SM
from common import D, cfg, payload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

INFO_BITS = (1, 7, 8, 58, 59, 250, 8186)
NCW = (1, 3, 5, 257)
PAD = 64
SENTINEL = 77
AMP = 8  # |LLR| of a clean coded bit in the noisy integer tests
# integer noise (std) per rate: near the code's threshold, so that the model
# itself decodes part of the codewords wrongly and the comparison is of the
# recursion and the tie rule, not of the payload
NOISE_STD = {F.R12: 10.0, F.R23: 7.0, F.R34: 5.5}


@functools.lru_cache(maxsize=None)
def modem():
    return M.Modem(D, 0)


def eff_ncw(nb, ncw):
    """info_bits = 8186 runs with at most 64 codewords (the model stays fast)."""
    return min(ncw, 64) if nb == 8186 else ncw


@functools.lru_cache(maxsize=None)
def info_bits_of(nb, ncw):
    return np.random.default_rng(1000 * nb + ncw).integers(0, 2, (ncw, nb), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def coded_of(nb, ncw, rate):
    return F.encode(info_bits_of(nb, ncw), rate)


@functools.lru_cache(maxsize=None)
def noisy_case(nb, ncw, rate):
    """(int8 LLRs (ncw, coded_bits), the model's bits, the sent bits)."""
    c = coded_of(nb, ncw, rate).astype(np.int64)
    rng = np.random.default_rng(7 + 31 * nb + ncw + 1000003 * rate)
    noise = np.rint(rng.normal(0.0, NOISE_STD[rate], c.shape)).astype(np.int64)
    llr = np.clip((1 - 2 * c) * AMP + noise, -127, 127).astype(np.int8)
    bits, _ = F.viterbi(llr.astype(np.int64), nb, rate)
    for a in (llr, bits):
        a.setflags(write=False)
    return llr, bits, info_bits_of(nb, ncw)


def sentinel_u8(n):
    return torch.full((n + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")


def run_decode(llr, nb, rate, fmt=M.LLR_I8, stride_slack=0, info_slack=0, ref=None, errs=None, stream=None,
               sync=True):
    """One ofdm_fec_decode launch on host LLRs (ncw, coded_bits). The LLR rows
    get `stride_slack` elements of +-127 garbage behind them. Returns the
    (ncw, ceil(nb/8)) output bytes after the sentinel and input checks."""
    ncw, cb = llr.shape
    assert cb == F.coded_bits(nb, rate)
    lstride = cb + stride_slack
    rows = np.empty((ncw, lstride), llr.dtype)
    rows[:, :cb] = llr
    rows[:, cb:] = (np.random.default_rng(5).integers(0, 2, (ncw, stride_slack)) * 254 - 127).astype(llr.dtype)
    d_llr = torch.from_numpy(rows).cuda()
    nbytes = (nb + 7) // 8
    istride = nbytes + info_slack
    out = sentinel_u8(ncw * istride)
    wsz = M.fec_workspace_size(ncw, nb)
    ws = torch.empty((wsz,), dtype=torch.uint8, device="cuda") if wsz else None
    d_ref = None
    if ref is not None:
        r = np.full((ncw, istride), 0xFF, np.uint8)  # bits past info_bits and slack bytes are set: not counted
        r[:, :nbytes] = ref
        if nb % 8:
            r[:, nbytes - 1] |= 0xFF >> (nb % 8)
        d_ref = torch.from_numpy(r).cuda()
    modem().fec_decode(d_llr, ncw, nb, rate, out, fmt=fmt, llr_stride=lstride, workspace=ws, info_stride=istride,
                       ref=d_ref, bit_errors=errs, stream=stream)
    if not sync:
        return out, (d_llr, ws, d_ref)
    torch.cuda.synchronize()
    return take_info(out, ncw, nbytes, istride, d_llr, rows)


def take_info(out, ncw, nbytes, istride, d_llr=None, rows=None):
    h = out.cpu().numpy()
    assert np.all(h[ncw * istride:] == SENTINEL), "the decoder wrote past its output"
    h = h[:ncw * istride].reshape(ncw, istride)
    assert np.all(h[:, nbytes:] == SENTINEL), "the decoder wrote between the codewords' outputs"
    if d_llr is not None:
        assert np.array_equal(d_llr.cpu().numpy().view(np.uint8), rows.view(np.uint8)), "the input was modified"
    return h[:, :nbytes]


# ------------------------------------------------------------------ encoder
@pytest.mark.parametrize("slack", [0, 3])
@pytest.mark.parametrize("rate", F.RATES)
@pytest.mark.parametrize("ncw", NCW)
@pytest.mark.parametrize("nb", INFO_BITS)
def test_encoder_equals_the_model(nb, ncw, rate, slack):
    info = info_bits_of(nb, ncw)
    nbytes = (nb + 7) // 8
    cb = F.coded_bits(nb, rate)
    cbytes = (cb + 7) // 8
    istride, cstride = nbytes + slack, cbytes + 2 * slack
    rows = np.random.default_rng(3).integers(0, 256, (ncw, istride), dtype=np.uint8)  # slack bytes: garbage
    rows[:, :nbytes] = F.pack(info)
    if nb % 8:
        rows[:, nbytes - 1] |= 0xFF >> (nb % 8)  # bits past info_bits are set and must be ignored
    d_in = torch.from_numpy(rows).cuda()
    out = sentinel_u8(ncw * cstride)
    modem().fec_encode(d_in, ncw, nb, rate, out, info_stride=istride, coded_stride=cstride)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert np.all(h[ncw * cstride:] == SENTINEL), "the encoder wrote past its output"
    h = h[:ncw * cstride].reshape(ncw, cstride)
    assert np.array_equal(d_in.cpu().numpy(), rows), "the input was modified"
    assert np.array_equal(h[:, :cbytes], F.pack(coded_of(nb, ncw, rate)))  # pad bits of the last byte are zero
    assert not h[:, cbytes:].any(), "bytes up to coded_stride must be zero"


def test_encoder_ignores_bits_past_info_bits():
    m = modem()
    for nb in (1, 7, 59, 250):
        nbytes = (nb + 7) // 8
        a = F.pack(info_bits_of(nb, 5))
        b = a.copy()
        b[:, nbytes - 1] |= 0xFF >> (nb % 8)
        assert not np.array_equal(a, b)
        outs = []
        for x in (a, b):
            cbytes = (F.coded_bits(nb, F.R34) + 7) // 8
            out = sentinel_u8(5 * cbytes)
            m.fec_encode(torch.from_numpy(x).cuda(), 5, nb, F.R34, out)
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
        assert np.array_equal(outs[0], outs[1])


# ------------------------------------------------------------------ decoder, int8
@pytest.mark.parametrize("slack", [0, 5])
@pytest.mark.parametrize("rate", F.RATES)
@pytest.mark.parametrize("ncw", NCW)
@pytest.mark.parametrize("nb", INFO_BITS)
def test_decoder_i8_equals_the_model(nb, ncw, rate, slack):
    ncw = eff_ncw(nb, ncw)
    llr, bits, sent = noisy_case(nb, ncw, rate)
    if ncw >= 64 and nb >= 58:
        assert np.any(bits != sent, axis=1).sum() >= 4, "the noise must make the model itself err on codewords"
    got = run_decode(llr, nb, rate, stride_slack=slack, info_slack=slack // 2)
    assert np.array_equal(got, F.pack(bits))


@pytest.mark.parametrize("nb", [122, 1018, 1019, 2042])
def test_decoder_i8_tile_and_survivor_storage_boundaries(nb):
    """T = 128 (two full tiles), and the lengths around the step count where
    the survivors move from LDS to the workspace."""
    for rate in F.RATES:
        llr, bits, _ = noisy_case(nb, 6, rate)
        assert np.array_equal(run_decode(llr, nb, rate), F.pack(bits))


@pytest.mark.parametrize("nb,ncw", [(59, 5), (250, 257), (8186, 3)])
def test_decoder_lds_pair_gather_variant(nb, ncw, monkeypatch):
    """OFDM_FEC_GATHER=lds (the A/B variant tools/coded_ber.py times): the
    same bits, int8 and float."""
    monkeypatch.setenv("OFDM_FEC_GATHER", "lds")
    for rate in F.RATES:
        llr, bits, _ = noisy_case(nb, ncw, rate)
        assert np.array_equal(run_decode(llr, nb, rate, stride_slack=1), F.pack(bits))
        li = np.clip(llr.astype(np.int64), -64, 64)
        if nb <= 250:
            got = run_decode(li.astype(np.float32), nb, rate, fmt=M.LLR_F32)
            assert np.array_equal(got, model_bytes(li, nb, rate))


def model_bytes(llr, nb, rate):
    bits, _ = F.viterbi(np.asarray(llr).astype(np.int64), nb, rate)
    return F.pack(bits)


@pytest.mark.parametrize("rate", F.RATES)
def test_decoder_i8_all_ties(rate):
    """All-zero LLRs: every add-compare-select is a tie."""
    for nb in (1, 58, 59, 250, 8186):
        llr = np.zeros((3, F.coded_bits(nb, rate)), np.int8)
        got = run_decode(llr, nb, rate)
        assert np.array_equal(got, model_bytes(llr, nb, rate))
        assert not got.any()  # the tie rule's path is the all-zero word (test_fec_model.py)


@pytest.mark.parametrize("rate", F.RATES)
def test_decoder_i8_metric_range(rate):
    """8186 bits of +127, of -127, and a noiseless +-127 codeword: the largest
    metrics an 8186-bit codeword can reach."""
    nb = 8186
    cb = F.coded_bits(nb, rate)
    c = coded_of(nb, 1, rate).astype(np.int64)
    llr = np.stack([np.full(cb, 127), np.full(cb, -127), (1 - 2 * c[0]) * 127]).astype(np.int8)
    got = run_decode(llr, nb, rate)
    assert np.array_equal(got, model_bytes(llr, nb, rate))
    assert np.array_equal(got[2], F.pack(info_bits_of(nb, 1))[0])


@pytest.mark.parametrize("rate", F.RATES)
def test_decoder_i8_single_nonzero_llr(rate):
    """LLRs that are 0 except one position, either sign: ties everywhere else."""
    nb = 58
    cb = F.coded_bits(nb, rate)
    llr = np.zeros((2 * cb, cb), np.int8)
    llr[np.arange(cb), np.arange(cb)] = 9
    llr[cb + np.arange(cb), np.arange(cb)] = -9
    got = run_decode(llr, nb, rate)
    ref = model_bytes(llr, nb, rate)
    assert np.array_equal(got, ref)
    assert ref.any(), "some single negative LLR must pull the path off the all-zero word"


# ------------------------------------------------------------------ decoder, f32
@pytest.mark.parametrize("rate", F.RATES)
@pytest.mark.parametrize("nb", [1, 7, 8, 58, 59, 250])
def test_decoder_f32_integer_valued_equals_the_model(nb, rate):
    """|L| <= 64 integers: float sums are exact, so the int model applies."""
    for ncw in (1, 5, 257):
        llr, _, _ = noisy_case(nb, ncw, rate)
        li = np.clip(llr.astype(np.int64), -64, 64)
        got = run_decode(li.astype(np.float32), nb, rate, fmt=M.LLR_F32, stride_slack=3)
        assert np.array_equal(got, model_bytes(li, nb, rate))


@pytest.mark.parametrize("rate", F.RATES)
@pytest.mark.parametrize("nb,ncw", [(59, 33), (250, 9), (8186, 3)])
def test_decoder_f32_real_valued_is_within_rounding_of_the_best_path(nb, ncw, rate):
    """The GPU's path, re-encoded, has a float64 metric >= the model's best
    minus T * 2^-23 * sum|L_n|: the bound on f32 accumulation error over the
    compared paths."""
    c = coded_of(nb, eff_ncw(nb, ncw), rate).astype(np.float64)
    rng = np.random.default_rng(11 + nb + rate)
    llr = ((1 - 2 * c) * 2.5 + rng.normal(0.0, NOISE_STD[rate] * 2.5 / AMP, c.shape)).astype(np.float32)
    got = run_decode(llr, nb, rate, fmt=M.LLR_F32)
    _, best = F.viterbi(llr.astype(np.float64), nb, rate)
    metric = F.path_metric(F.unpack(got, nb), llr.astype(np.float64), rate)
    bound = (nb + 6) * 2.0 ** -23 * np.abs(llr.astype(np.float64)).sum(axis=1)
    print("f32 path metric deficit (max)", float((best - metric).max()), "bound (min)", float(bound.min()))
    assert np.all(metric >= best - bound)


# ------------------------------------------------------------------ counters, streams, errors
def test_bit_errors_accumulate_over_two_launches():
    total = 0
    errs = torch.zeros((1,), dtype=torch.int64, device="cuda")
    for nb, ncw, rate in ((250, 257, F.R34), (59, 5, F.R12), (8186, 3, F.R23)):
        llr, bits, sent = noisy_case(nb, eff_ncw(nb, ncw), rate)
        got = run_decode(llr, nb, rate, info_slack=2, ref=F.pack(sent), errs=errs)
        assert np.array_equal(got, F.pack(bits))
        total += int((bits != sent).sum())
        assert int(errs.item()) == total
    assert total > 0


def test_two_launches_on_a_side_stream():
    nb, ncw, rate = 8186, 5, F.R12
    llr, bits, _ = noisy_case(nb, ncw, rate)
    llr2 = np.ascontiguousarray(llr[::-1])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        o1, keep1 = run_decode(llr, nb, rate, stream=s, sync=False)
        o2, keep2 = run_decode(llr2, nb, rate, stream=s, sync=False)
    s.synchronize()
    nbytes = (nb + 7) // 8
    assert np.array_equal(take_info(o1, ncw, nbytes, nbytes), F.pack(bits))
    assert np.array_equal(take_info(o2, ncw, nbytes, nbytes), F.pack(bits)[::-1])


def test_invalid_arguments():
    m = modem()
    L = M.lib()
    st = torch.cuda.current_stream().cuda_stream
    nb, ncw = 250, 4
    cb = F.coded_bits(nb, F.R12)
    info = torch.zeros((ncw * 32,), dtype=torch.uint8, device="cuda")
    coded = torch.zeros((ncw * 64,), dtype=torch.uint8, device="cuda")
    llr = torch.zeros((ncw * cb + 8,), dtype=torch.float32, device="cuda")
    big = 8186
    big_llr = torch.zeros((2 * F.coded_bits(big, F.R12),), dtype=torch.int8, device="cuda")
    big_out = torch.zeros((2 * 1024,), dtype=torch.uint8, device="cuda")
    wsz = M.fec_workspace_size(2, big)
    assert wsz > 0 and M.fec_workspace_size(ncw, nb) == 0
    ws = torch.zeros((wsz + 16,), dtype=torch.uint8, device="cuda")

    def enc(h=m.h, i=info.data_ptr(), istr=32, n=ncw, bits=nb, rate=F.R12, c=coded.data_ptr(), cstr=64):
        return L.ofdm_fec_encode(h, i, istr, n, bits, rate, c, cstr, st)

    def dec(h=m.h, l=llr.data_ptr(), fmt=M.LLR_F32, lstr=cb, n=ncw, bits=nb, rate=F.R12, w=None, wb=0,
            o=info.data_ptr(), ostr=32, ref=None, be=None):
        return L.ofdm_fec_decode(h, l, fmt, lstr, n, bits, rate, w, wb, o, ostr, ref, be, st)

    def decbig(w=ws.data_ptr(), wb=wsz):
        return dec(l=big_llr.data_ptr(), fmt=M.LLR_I8, lstr=F.coded_bits(big, F.R12), n=2, bits=big, w=w, wb=wb,
                   o=big_out.data_ptr(), ostr=1024)

    assert enc() == 0 and dec() == 0 and decbig() == 0
    assert enc(n=0) == 0 and dec(n=0) == 0  # nothing launched
    assert enc(h=None) == -1 and enc(i=None) == -1 and enc(c=None) == -1
    assert dec(h=None) == -1 and dec(l=None) == -1 and dec(o=None) == -1
    for call in (enc, dec):
        assert call(rate=3) == -1 and call(rate=-1) == -1
        assert call(bits=0) == -1 and call(bits=(1 << 20) + 1) == -1
    assert dec(fmt=2) == -1 and dec(fmt=-1) == -1
    assert enc(istr=31) == -1 and enc(cstr=63) == -1  # 250 bits: 32 bytes in, 512 coded bits: 64 bytes out
    assert dec(lstr=cb - 1) == -1 and dec(ostr=31) == -1
    assert dec(l=llr.data_ptr() + 2) == -1                      # F32 input not 4-byte aligned
    assert dec(fmt=M.LLR_I8, l=llr.data_ptr() + 1) == 0         # int8 input: any address
    assert decbig(w=None) == -1                                 # the size query is non-zero: NULL workspace
    assert decbig(wb=wsz - 1) == -1 and decbig(wb=0) == -1      # too small
    assert decbig(w=ws.data_ptr() + 8) == -1                    # not 16-byte aligned
    assert dec(w=None, wb=0) == 0                               # short codewords need none
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end
E2E = {"D_k2": (cfg(D, mod_type=2), 0.5, 8.0), "D": (D, 0.22, 40.0)}


@functools.lru_cache(maxsize=None)
def e2e_cpu(name):
    """The link on the CPU: oracle tx + awgn + rx points, the soft model's int8
    LLRs, the Viterbi model. Returns what the GPU run needs."""
    p, rel_noise, scale = E2E[name]
    g = O.geometry(p)
    nf = 4
    nb = M.fec_max_info_bits(g["bytes_per_frame"] * 8, F.R12)
    info = F.unpack(payload(nf * ((nb + 7) // 8), 21).reshape(nf, -1), nb)
    coded = np.zeros((nf, g["bytes_per_frame"]), np.uint8)
    packed = F.pack(F.encode(info, F.R12))
    coded[:, :packed.shape[1]] = packed
    x = O.tx_batch(p, coded.reshape(-1), nf)
    power = float(np.mean(np.abs(x) ** 2))
    iq = O.awgn(x, np.sqrt(power) * rel_noise, seed=5)
    E, hard, _ = O.rx_batch(p, iq, nf, g["message_len"])
    L = np.clip(np.rint(SM.ref_llr(p["mod_type"], E.reshape(nf, -1), scale)), -127, 127).astype(np.int64)
    bits, _ = F.viterbi(L.reshape(nf, -1), nb, F.R12)
    hard_errors = int(np.unpackbits(hard.reshape(nf, -1) ^ coded, axis=1).sum())
    return p, nf, nb, info, coded, iq, scale, int((bits != info).sum()), hard_errors


@pytest.mark.parametrize("name", list(E2E))
def test_coded_link_end_to_end(name):
    """fec_encode -> oracle tx + awgn -> rx_soft int8 -> fec_decode, one
    rate-1/2 codeword per frame, 4 frames. Noise std relative to the rms of
    the tx samples, chosen on the CPU (e2e_cpu): D_k2 (QPSK, 2042 info bits)
    0.5 with LLR scale 8; D (16-QAM, 4090 info bits) 0.22 with scale 40.
    CPU-side counts at these values: the model decodes every codeword to the
    payload (0 info bit errors of 8168 / 16360), while the hard decisions hold
    D_k2: 169, D: 303 bit errors among the 16384 / 32768 coded-frame bits."""
    p, nf, nb, info, coded, iq, scale, model_errors, hard_errors = e2e_cpu(name)
    assert model_errors == 0 and hard_errors > 0
    g = O.geometry(p)
    k = p["mod_type"]
    m = M.Modem(p, 0)
    nbytes = (nb + 7) // 8
    d_info = torch.from_numpy(F.pack(info)).cuda()
    d_coded = sentinel_u8(nf * g["bytes_per_frame"])
    m.fec_encode(d_info, nf, nb, F.R12, d_coded, coded_stride=g["bytes_per_frame"])
    torch.cuda.synchronize()
    assert np.array_equal(d_coded.cpu().numpy()[:nf * g["bytes_per_frame"]], coded.reshape(-1))
    d_iq = torch.from_numpy(iq).cuda()
    n_llr = nf * g["npts"] * k
    llr = torch.full((n_llr + PAD,), SENTINEL, dtype=torch.int8, device="cuda")
    hard = torch.zeros((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
    e_hard = torch.zeros((1,), dtype=torch.int64, device="cuda")
    e_dec = torch.zeros((1,), dtype=torch.int64, device="cuda")
    m.rx_soft(d_iq, nf, llr, scale, M.LLR_I8, bytes_out=hard, ref=d_coded, bit_errors=e_hard)
    wsz = M.fec_workspace_size(nf, nb)
    ws = torch.empty((wsz,), dtype=torch.uint8, device="cuda") if wsz else None
    out = sentinel_u8(nf * nbytes)
    m.fec_decode(llr, nf, nb, F.R12, out, fmt=M.LLR_I8, llr_stride=g["npts"] * k, workspace=ws, ref=d_info,
                 bit_errors=e_dec)
    torch.cuda.synchronize()
    assert np.array_equal(take_info(out, nf, nbytes, nbytes), F.pack(info))
    assert int(e_hard.item()) > 0
    assert int(e_dec.item()) == 0
    m.close()
