"""Interleaver and scrambler on the GPU: ofdm_interleave_bits,
ofdm_interleave_llr and ofdm_scramble against the numpy model of
tests/interleave_model.py bit for bit, every error return, stream order, graph
capture, and the coded link through a notch end to end.

Every output buffer carries sentinels before and past the bytes a launch may
write (and, with stride slack, between them); every input is checked
unmodified."""
import ctypes as C
import functools

import numpy as np
import pytest

import fec_model as F
import interleave_model as IM
import oracle as O
from common import ALL_CONFIGS
from test_gpu_graph import replay_protocol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

# the smallest block, a non-power-of-two block, a column count other than 16,
# every s, several blocks per workgroup, and the largest block
BLOCKS = ((8, 1, 1), (8, 8, 1), (32, 16, 1), (48, 16, 1), (96, 16, 3), (192, 12, 4), (256, 16, 2), (1024, 16, 2),
          (1536, 16, 3), (8192, 16, 2), (32768, 16, 4))
KINDS = ("bits", "i8", "f32")
OFFSETS = (0, 1, 4)  # elements from a 16-byte boundary: 1 and 4 take the narrow loads and stores
PAD = 64
SENTINEL = 77


@functools.lru_cache(maxsize=None)
def modem(name="D"):
    return M.Modem(ALL_CONFIGS[name], 0)


def nblocks_of(n):
    return (1, 3, 5) if n >= 8192 else (1, 3, 257)


@functools.lru_cache(maxsize=None)
def case(kind, n, c, s, nblocks):
    """(input units, forward result, inverse result) of one shape; the units
    are bytes of packed bits, int8, or the raw words of float32."""
    rng = np.random.default_rng(n + 7 * c + 31 * s + 1009 * nblocks)
    if kind == "bits":
        x = rng.integers(0, 256, nblocks * n // 8, dtype=np.uint8)
        b = np.unpackbits(x)
        res = [np.packbits(f(b, n, c, s)) for f in (IM.interleave, IM.deinterleave)]
    else:
        x = (rng.integers(0, 256, nblocks * n, dtype=np.uint8) if kind == "i8"
             else rng.integers(0, 1 << 32, nblocks * n, dtype=np.uint32))  # every bit pattern, NaNs among them
        res = [f(x, n, c, s) for f in (IM.interleave, IM.deinterleave)]
    for a in (x, *res):
        a.setflags(write=False)
    return x, res[0], res[1]


def offset_buffer(nbytes, off_bytes, fill=None):
    """(whole uint8 tensor, its live slice): `nbytes` live bytes off_bytes past
    a 16-byte boundary, sentinels around them."""
    raw = torch.full((16 + off_bytes + nbytes + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    live = raw[16 + off_bytes:16 + off_bytes + nbytes]
    if fill is not None:
        live.copy_(torch.from_numpy(fill.view(np.uint8).copy()))
    return raw, live


def launch(kind, src, nblocks, block, direction, dst, stream=None):
    m = modem()
    if kind == "bits":
        m.interleave_bits(src, nblocks, dst, direction, block=block, stream=stream)
    else:
        m.interleave_llr(src, nblocks, dst, direction, fmt=M.LLR_I8 if kind == "i8" else M.LLR_F32, block=block,
                         stream=stream)


def run_il(kind, x, nblocks, block, direction, off=0):
    """One launch on host units x; returns the output units after the
    sentinel and input checks."""
    es = x.itemsize
    raw_in, d_in = offset_buffer(x.nbytes, off * es, x)
    raw_out, d_out = offset_buffer(x.nbytes, off * es)
    before = raw_in.clone()
    launch(kind, d_in, nblocks, block, direction, d_out)
    torch.cuda.synchronize()
    assert torch.equal(raw_in, before), "the input was modified"
    h = raw_out.cpu().numpy()
    lo = 16 + off * es
    assert np.all(h[:lo] == SENTINEL) and np.all(h[lo + x.nbytes:] == SENTINEL), "wrote outside the output"
    return h[lo:lo + x.nbytes].view(x.dtype)


# ------------------------------------------------------------------ the permutation
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,c,s", BLOCKS)
def test_kernels_equal_the_model(n, c, s, kind):
    for nblocks in nblocks_of(n):
        x, fwd, inv = case(kind, n, c, s, nblocks)
        for off in OFFSETS:
            got = run_il(kind, x, nblocks, (n, c, s), M.IL_FORWARD, off)
            assert np.array_equal(got, fwd), ("forward", nblocks, off)
            got = run_il(kind, x, nblocks, (n, c, s), M.IL_INVERSE, off)
            assert np.array_equal(got, inv), ("inverse", nblocks, off)


@pytest.mark.parametrize("kind", KINDS)
def test_inverse_after_forward_is_the_identity(kind):
    for n, c, s in BLOCKS:
        nblocks = nblocks_of(n)[1]
        x, _, _ = case(kind, n, c, s, nblocks)
        d_x = torch.from_numpy(x.view(np.uint8).copy()).cuda()
        mid, back = torch.empty_like(d_x), torch.empty_like(d_x)
        launch(kind, d_x, nblocks, (n, c, s), M.IL_FORWARD, mid)
        launch(kind, mid, nblocks, (n, c, s), M.IL_INVERSE, back)
        torch.cuda.synchronize()
        assert torch.equal(back, d_x), (n, c, s)
        assert not torch.equal(mid, d_x) or n == 8


def test_f32_moves_nan_payloads_and_negative_zero_bit_for_bit():
    n, c, s = 256, 16, 2
    specials = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFBFFFFF, 0x80000000, 0x00000000, 0x7F800000,
                         0xFF800000, 0x00000001, 0x80000001], np.uint32)
    x = np.resize(specials, 3 * n)
    assert np.isnan(x.view(np.float32)).sum() >= n and np.signbit(x.view(np.float32)[4])
    for off in OFFSETS:
        assert np.array_equal(run_il("f32", x, 3, (n, c, s), M.IL_FORWARD, off), IM.interleave(x, n, c, s))
        assert np.array_equal(run_il("f32", x, 3, (n, c, s), M.IL_INVERSE, off), IM.deinterleave(x, n, c, s))


def test_interleave_default_on_every_config():
    assert len(ALL_CONFIGS) == 16
    for name, p in ALL_CONFIGS.items():
        k = p["mod_type"]
        m = modem(name)
        assert m.interleave_default() == (p["num_data_subc"] * k, 16, max(k // 2, 1)), name
        assert IM.valid(*m.interleave_default()), name
    n = C.c_size_t(777)
    L, h = M.lib(), modem().h
    assert L.ofdm_interleave_default(h, None, C.byref(n), C.byref(n)) == -1
    assert L.ofdm_interleave_default(h, C.byref(n), None, C.byref(n)) == -1
    assert L.ofdm_interleave_default(h, C.byref(n), C.byref(n), None) == -1
    assert n.value == 777


def test_default_block_is_what_the_modem_methods_use():
    m = modem("N128_k4_s3")
    n, c, s = m.interleave_default()
    x, fwd, inv = case("i8", n, c, s, 3)
    d_x = torch.from_numpy(x.copy()).cuda()
    out = torch.empty_like(d_x)
    m.interleave_llr(d_x, 3, out, M.IL_FORWARD)
    assert np.array_equal(out.cpu().numpy(), fwd)
    m.interleave_llr(d_x, 3, out)  # the LLR call's default direction is the receiver's
    assert np.array_equal(out.cpu().numpy(), inv)
    xb, fb, _ = case("bits", n, c, s, 3)
    outb = torch.empty((xb.size,), dtype=torch.uint8, device="cuda")
    m.interleave_bits(torch.from_numpy(xb.copy()).cuda(), 3, outb)  # the bit call's default is the transmitter's
    assert np.array_equal(outb.cpu().numpy(), fb)


# ------------------------------------------------------------------ the scrambler
NBITS = (1, 7, 8, 127, 128, 1000, 8186)
NCW = (1, 3, 257)


@functools.lru_cache(maxsize=None)
def scr_case(nbits, ncw):
    rng = np.random.default_rng(100 * nbits + ncw)
    bits = rng.integers(0, 2, (ncw, nbits), dtype=np.uint8)
    seeds = rng.integers(0, 256, ncw, dtype=np.uint8)
    seeds[:3] = (0, 128, 255)[:ncw]  # values the device reduces
    return bits, seeds


@functools.lru_cache(maxsize=None)
def scr_sequences(nbits):
    """Row v: the model's sequence of seed v (row 0 unused). The model runs for
    two periods, which must agree; longer sequences repeat the first."""
    rows = [np.zeros(nbits, np.uint8)]
    for v in range(1, 128):
        q = IM.scramble_sequence(v, 254)
        assert np.array_equal(q[:127], q[127:])
        rows.append(np.resize(q[:127], nbits))
    return np.stack(rows)


def model_scramble(bits, seeds):
    seeds = np.broadcast_to(np.asarray(seeds), (bits.shape[0],))
    idx = np.array([IM.reduce_seed(v) for v in seeds])
    return bits ^ scr_sequences(bits.shape[1])[idx]


def run_scramble(bits, seed=127, seeds=None, slack=0, in_place=False, oslack=None):
    """One launch on (ncw, nbits) bits. The bits past nbits of each input row's
    last byte are set and the rows have `slack` bytes of stride slack (garbage
    in the input, sentinels in the output). Returns the (ncw, nbytes) bytes."""
    ncw, nbits = bits.shape
    nbytes = (nbits + 7) // 8
    stride = nbytes + slack
    rows = np.random.default_rng(9).integers(0, 256, (ncw, stride), dtype=np.uint8)
    rows[:, :nbytes] = F.pack(bits)
    if nbits % 8:
        rows[:, nbytes - 1] |= 0xFF >> (nbits % 8)
    if in_place:
        rows[:, nbytes:] = SENTINEL
    d_in = torch.from_numpy(rows.reshape(-1)).cuda()
    ostride = stride if in_place else nbytes + (2 * slack if oslack is None else oslack)
    out = d_in if in_place else torch.full((ncw * ostride + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_seeds = torch.from_numpy(seeds).cuda() if seeds is not None else None
    modem().scramble(d_in, ncw, nbits, out, seed=seed, seeds=d_seeds, in_stride=stride, out_stride=ostride)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy(), rows.reshape(-1)), "the input was modified"
        assert np.all(h[ncw * ostride:] == SENTINEL), "wrote past the output"
    h = h[:ncw * ostride].reshape(ncw, ostride)
    assert np.all(h[:, nbytes:] == SENTINEL), "wrote between the codewords"
    return h[:, :nbytes]


@pytest.mark.parametrize("ncw", NCW)
@pytest.mark.parametrize("nbits", NBITS)
def test_scrambler_equals_the_model(nbits, ncw):
    bits, seeds = scr_case(nbits, ncw)
    for seed in (127, 1, 93):
        got = run_scramble(bits, seed=seed)
        assert np.array_equal(got, F.pack(model_scramble(bits, seed)))  # the pad bits of the last byte are zero
    got = run_scramble(bits, seed=0, seeds=seeds, slack=3)  # the scalar seed is ignored
    assert np.array_equal(got, F.pack(model_scramble(bits, seeds)))


def test_scrambler_word_path_with_a_tail():
    """Strides that are multiples of 4 with codewords that are not: the last
    1 to 3 bytes of a codeword leave byte by byte, and the slack stays."""
    for nbits, ncw in ((7, 3), (127, 257), (1000, 257), (1000 + 16, 3), (8186 - 16, 3)):
        bits, seeds = scr_case(nbits, ncw)
        nbytes = (nbits + 7) // 8
        slack = 4 - nbytes % 4
        got = run_scramble(bits, seeds=seeds, slack=slack, oslack=slack + 4)
        assert np.array_equal(got, F.pack(model_scramble(bits, seeds)))
        got = run_scramble(bits, seeds=seeds, slack=slack, in_place=True)
        assert np.array_equal(got, F.pack(model_scramble(bits, seeds)))


def test_scrambler_in_place_and_self_inverse():
    for nbits, ncw in ((1000, 3), (8186, 257), (7, 3)):
        bits, seeds = scr_case(nbits, ncw)
        once = run_scramble(bits, seeds=seeds, slack=2, in_place=True)
        assert np.array_equal(once, F.pack(model_scramble(bits, seeds)))
        twice = run_scramble(F.unpack(once, nbits), seeds=seeds, in_place=True)
        assert np.array_equal(twice, F.pack(bits))


def test_scrambler_sequence_of_seed_127():
    zeros = np.zeros((1, 254), np.uint8)
    got = F.unpack(run_scramble(zeros), 254)[0]
    assert "".join(map(str, got[:32])) == "00001110" "11110010" "11001001" "00000010"
    assert np.array_equal(got[:127], got[127:]) and int(got[:127].sum()) == 64


# ------------------------------------------------------------------ errors
def test_invalid_arguments_launch_nothing():
    m, L = modem(), M.lib()
    st = torch.cuda.current_stream().cuda_stream
    n, c, s, nblocks = 192, 16, 2, 4
    src = torch.full((nblocks * n * 4 + 64,), 5, dtype=torch.uint8, device="cuda")
    dst = torch.full((nblocks * n * 4 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    seeds = torch.full((8,), 3, dtype=torch.uint8, device="cuda")

    def bits(h=m.h, i=src.data_ptr(), nb=nblocks, n=n, c=c, s=s, d=0, o=dst.data_ptr()):
        return L.ofdm_interleave_bits(h, i, nb, n, c, s, d, o, st)

    def llr(h=m.h, i=src.data_ptr(), fmt=M.LLR_I8, nb=nblocks, n=n, c=c, s=s, d=1, o=dst.data_ptr()):
        return L.ofdm_interleave_llr(h, i, fmt, nb, n, c, s, d, o, st)

    def scr(h=m.h, i=src.data_ptr(), istr=24, ncw=4, nbits=192, seed=127, sd=None, o=dst.data_ptr(), ostr=24):
        return L.ofdm_scramble(h, i, istr, ncw, nbits, seed, sd, o, ostr, st)

    for call in (bits, llr):
        assert call(h=None) == -1 and call(i=None) == -1 and call(o=None) == -1
        assert call(d=2) == -1 and call(d=-1) == -1
        for bad in ((0, 1, 1), (4, 1, 1), (12, 1, 1), (190, 1, 1), (32776, 8, 1), (192, 0, 1), (192, 5, 1),
                    (192, 384, 1), (192, 16, 0), (192, 16, 5), (192, 16, 24)):
            assert call(n=bad[0], c=bad[1], s=bad[2]) == -1, bad
        assert call(o=src.data_ptr()) == -1                                  # in == out
        assert call(o=src.data_ptr() + 8) == -1 and call(i=dst.data_ptr() + 8) == -1  # partial overlap
        assert call(nb=0) == 0                                               # nothing launched
    assert llr(fmt=2) == -1 and llr(fmt=-1) == -1
    assert llr(fmt=M.LLR_F32, i=src.data_ptr() + 2) == -1 and llr(fmt=M.LLR_F32, o=dst.data_ptr() + 1) == -1
    assert scr(h=None) == -1 and scr(i=None) == -1 and scr(o=None) == -1
    assert scr(nbits=0) == -1 and scr(istr=23) == -1 and scr(ostr=23) == -1
    assert scr(seed=0) == -1 and scr(seed=128) == -1
    assert scr(o=src.data_ptr(), ostr=25, istr=24) == -1                     # in place with unequal strides
    assert scr(ncw=0) == 0
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all()) and bool((src == 5).all()), "an invalid call launched something"
    # and the same calls with valid arguments do write
    assert llr(fmt=M.LLR_I8, i=src.data_ptr() + 1) == 0 and scr(seed=0, sd=seeds.data_ptr()) == 0 and bits() == 0
    assert llr(fmt=M.LLR_F32) == 0
    torch.cuda.synchronize()
    assert not bool((dst[:nblocks * n * 4] == SENTINEL).all()) and bool((dst[nblocks * n * 4:] == SENTINEL).all())


# ------------------------------------------------------------------ the coded link through a notch
class NotchLink:
    """tx: scramble, fec_encode (coded_stride = bytes_per_frame), interleave,
    tx_modulate without noise. rx: rx_soft (int8, scale 8), the LLRs of
    `count` carriers from `first` of every symbol zeroed with a torch slice,
    deinterleave, fec_decode, descramble. One codeword per frame."""

    def __init__(self, name, rate, first, count, nf=16, interleaved=True):
        p = ALL_CONFIGS[name]
        self.m, self.g, self.k, self.nf, self.rate = modem(name), O.geometry(p), p["mod_type"], nf, rate
        self.S, self.Dc = p["num_symb"], p["num_data_subc"]
        self.first, self.count, self.interleaved = first, count, interleaved
        g, u8 = self.g, torch.uint8
        self.cap = g["bytes_per_frame"] * 8
        assert self.cap == self.S * self.Dc * self.k
        self.nb = M.fec_max_info_bits(self.cap, rate)
        self.nbytes = (self.nb + 7) // 8
        self.info = torch.zeros((nf * self.nbytes,), dtype=u8, device="cuda")
        self.seeds = torch.from_numpy((np.arange(nf) * 37 % 256).astype(np.uint8)).cuda()
        self.scr = torch.empty_like(self.info)
        self.coded = torch.empty((nf * g["bytes_per_frame"],), dtype=u8, device="cuda")
        self.sent = torch.empty_like(self.coded)
        self.iq = torch.empty((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
        self.llr = torch.empty((nf * self.cap,), dtype=torch.int8, device="cuda")
        self.dellr = torch.empty_like(self.llr)
        self.dec = torch.empty_like(self.info)
        self.out = torch.empty((nf * self.nbytes + PAD,), dtype=u8, device="cuda")
        wsz = M.fec_workspace_size(nf, self.nb)
        self.ws = torch.empty((wsz,), dtype=u8, device="cuda") if wsz else None

    def payload(self, seed):
        bits = np.random.default_rng(seed).integers(0, 2, (self.nf, self.nb), dtype=np.uint8)
        return F.pack(bits)

    def load(self, seed):
        self.info.copy_(torch.from_numpy(self.payload(seed).reshape(-1)))

    def run(self):
        m, nf, nsym = self.m, self.nf, self.nf * self.S
        m.scramble(self.info, nf, self.nb, self.scr, seeds=self.seeds)
        m.fec_encode(self.scr, nf, self.nb, self.rate, self.coded, coded_stride=self.g["bytes_per_frame"])
        if self.interleaved:
            m.interleave_bits(self.coded, nsym, self.sent, M.IL_FORWARD)
        m.tx(self.coded if not self.interleaved else self.sent, nf, self.iq)
        m.rx_soft(self.iq, nf, self.llr, 8.0, M.LLR_I8)
        self.llr.view(nsym, self.Dc, self.k)[:, self.first:self.first + self.count, :] = 0
        if self.interleaved:
            m.interleave_llr(self.llr, nsym, self.dellr, M.IL_INVERSE, fmt=M.LLR_I8)
        m.fec_decode(self.dellr if self.interleaved else self.llr, nf, self.nb, self.rate, self.dec, fmt=M.LLR_I8,
                     llr_stride=self.cap, workspace=self.ws)
        m.scramble(self.dec, nf, self.nb, self.out, seeds=self.seeds)

    def wrong(self, seed):
        torch.cuda.synchronize()
        h = self.out.cpu().numpy()
        assert np.all(h[self.nf * self.nbytes:] == SENTINEL)
        got = h[:self.nf * self.nbytes].reshape(self.nf, self.nbytes)
        return int(np.any(got != self.payload(seed), axis=1).sum())


@pytest.mark.parametrize("rate", [F.R12, F.R23])
def test_notched_link_end_to_end(rate):
    """N128_k4_s3 (D = 64, 16-QAM, 3 symbols), carriers 21..25 of every symbol
    erased: every payload comes back through the interleaver, and the same
    chain without the two interleave calls loses codewords (the model of
    test_interleave_model.py loses all 16)."""
    link = NotchLink("N128_k4_s3", rate, 21, 5)
    link.load(1)
    link.out.fill_(SENTINEL)
    link.run()
    assert link.wrong(1) == 0
    control = NotchLink("N128_k4_s3", rate, 21, 5, interleaved=False)
    control.load(1)
    control.out.fill_(SENTINEL)
    control.run()
    lost = control.wrong(1)
    print("control leg: codewords lost", lost, "of", control.nf)
    assert lost >= 1, "the control leg has no errors: the test no longer shows anything"


def test_notched_link_on_config_D():
    link = NotchLink("D", F.R12, 21, 6)
    link.load(1)
    link.out.fill_(SENTINEL)
    link.run()
    assert link.wrong(1) == 0


def test_chain_on_a_side_stream_without_intermediate_syncs():
    link = NotchLink("N128_k4_s3", F.R23, 21, 5)
    link.load(4)
    link.out.fill_(SENTINEL)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        link.run()
        link.load(5)  # stream order: overwrites the input behind the first run
        first = link.out.clone()
        link.run()
    s.synchronize()
    assert link.wrong(5) == 0
    link.out.copy_(first)
    assert link.wrong(4) == 0


def test_graph_capture_of_the_full_chain():
    """test_gpu_graph.py's protocol: replay 1 equals the eager run, replay 2 on
    overwritten inputs equals a fresh eager run; both decode to the payload."""
    link = NotchLink("N128_k4_s3", F.R12, 21, 5)
    n_out = link.nf * link.nbytes
    outs = {"out": link.out, "llr": link.dellr, "sent": link.sent}
    live = {"out": n_out, "llr": link.dellr.numel(), "sent": link.sent.numel()}
    _, _, r1, r2, _ = replay_protocol(link.run, lambda c: link.load(10 + c), outs, live)
    assert np.array_equal(r1["out"][:n_out], link.payload(10).reshape(-1))
    assert np.array_equal(r2["out"][:n_out], link.payload(11).reshape(-1))
