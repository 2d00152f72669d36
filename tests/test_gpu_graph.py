"""hipGraph capture and replay of the batched entry points (the header's
"capturable"): each chain is captured once into a torch.cuda.CUDAGraph on one
stream (linear chains only: no forks, side streams or events), then replayed.

Protocol of every chain (replay_protocol): the calls run once eagerly with the
capture's sizes (module load, the LDS opt-in and the documented first-call
scratch allocations happen there), are captured, and
  - replay 1 on unchanged inputs equals the eager run bit for bit;
  - the inputs are overwritten in place, replay 2 equals a fresh eager run on
    the new data bit for bit and the CPU model / oracle at the eager tests'
    bars (1e-10 rx and flat kernels, 1e-9 behind the sync chain; bytes, int8
    LLRs and decoded bits as the eager tests take them);
  - every output is refilled with sentinels before each run, so nothing of an
    earlier replay can pass for a result, and the sentinels past each
    output's end (and in stride gaps) must survive;
  - bit_errors, an atomic accumulation, holds the sum of the replays' model
    counts.
A replay has no host code between two launches, so a per-launch device
counter (the rx frame queue, t2_scan's scratch, find_preamble's completion
counters) that a launch left dirty fails the next replay.

Not captured: ofdm_rx_stream* (the host waits for the walk's status word to
return the frame count) and ofdm_preamble_corr (stages its start index from
pageable host memory and synchronises the stream): both synchronise by
design, which a capture forbids."""
import functools

import numpy as np
import pytest

import fec_model as F
import oracle as O
import soft_model as SM
from common import ALL_CONFIGS, G, assert_int16_match, golden, payload, rel_err
from test_gpu_decision_boundary import smith_div
from test_gpu_sync import _impaired_frames

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

TOL = 1e-10        # test_gpu_parity.py's bar for rx / tx / the flat FFT kernels
TOL_SYNC = 1e-9    # test_gpu_sync.py's bar behind the sync chain
PAD = 64           # sentinel elements past every output
SENT_INT = 77
SENT_F = 9.0


@functools.lru_cache(maxsize=None)
def modem(name):
    return M.Modem(ALL_CONFIGS[name], 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def out_buf(n, dtype):
    return torch.empty((n + PAD,), dtype=dtype, device="cuda")


def fill_sentinel(t):
    if t.is_complex():
        t.fill_(complex(SENT_F, SENT_F))
    else:
        t.fill_(SENT_F if t.is_floating_point() else SENT_INT)


def is_sentinel(t):
    if t.is_complex():
        t = torch.view_as_real(t)
    return bool((t == (SENT_F if t.is_floating_point() else SENT_INT)).all())


def bits(t):
    """The tensor's bit patterns (equality of these is bit-for-bit equality)."""
    if t.is_complex():
        t = torch.view_as_real(t)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t


def load(t, a):
    """Overwrite an input tensor in place (its address is in the graph)."""
    src = torch.from_numpy(np.ascontiguousarray(a))
    assert src.shape == t.shape and src.dtype == t.dtype
    t.copy_(src)


def persistent_nf():
    """test_gpu_soft.py's test_persistent_loop: every workgroup takes several
    frames from the queue counter."""
    return 3 * 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5


def replay_protocol(run, load_case, outs, live, counters=()):
    """The capture / replay protocol of the module docstring.
    run(): the chain's calls (stream=None: torch's current stream);
    load_case(c): writes data set c (0, 1) into the input tensors in place;
    outs: {name: output tensor}, live: {name: elements the chain may write};
    counters: accumulating u64 counters, zeroed after the capture.
    Returns (graph, capture stream, host copies of replay 1's and replay 2's
    outputs, the counters' values after the two replays)."""

    def reset():
        for t in outs.values():
            fill_sentinel(t)

    def snap(what):
        torch.cuda.synchronize()
        for k, t in outs.items():
            assert is_sentinel(t[live[k]:]), f"{what}: the chain wrote past the end of {k}"
        return {k: t.clone() for k, t in outs.items()}

    def assert_same(a, b, what):
        for k in outs:
            assert torch.equal(bits(a[k]), bits(b[k])), f"{what}: output {k} differs"

    load_case(0)
    reset()
    run()
    eager0 = snap("eager run")
    for k, t in outs.items():
        assert not is_sentinel(t[:live[k]]), f"the eager run wrote nothing to {k}"
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    reset()
    with torch.cuda.graph(g, stream=s):
        run()
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert is_sentinel(t), f"the capture itself ran something that wrote {k}"
    for c in counters:
        c.zero_()
    g.replay()
    r1 = snap("replay 1")
    assert_same(r1, eager0, "replay 1 against the eager run")
    load_case(1)
    reset()
    g.replay()
    r2 = snap("replay 2")
    counts = [int(c.item()) for c in counters]
    reset()
    run()
    eager1 = snap("eager run on the new inputs")
    assert_same(r2, eager1, "replay 2 against an eager run on the new inputs")
    differs = [k for k in outs if not torch.equal(bits(r1[k]), bits(r2[k]))]
    assert differs, "the second data set must change some output"
    return g, s, {k: host(v) for k, v in r1.items()}, {k: host(v) for k, v in r2.items()}, counts


@functools.lru_cache(maxsize=None)
def tx_rms(name):
    p = ALL_CONFIGS[name]
    x = O.tx_batch(p, payload(O.geometry(p)["bytes_per_frame"], 1), 1)
    return float(np.sqrt(np.mean(np.abs(x) ** 2)))


# ------------------------------------------------------------------ 1. coded link
LINK_SEED = 12345
LINK_SCALE = 8.0


@pytest.mark.parametrize("name,rate,persistent", [("N64_k1", F.R12, False), ("N64_k1", F.R12, True),
                                                  ("N64_k1", F.R34, False), ("D_qpsk", F.R12, False)])
def test_coded_link(name, rate, persistent):
    """fec_encode -> tx (fused AWGN, fixed seed) -> rx_soft (int8, frame_scale
    in device memory, hard bytes counted against the coded bytes) ->
    fec_decode (counted against the info bytes), one codeword per frame.
    N64_k1 carries 26 info bits at rate 1/2; D_qpsk carries 2042 (>= 1019: the
    survivors live in the caller's workspace). Between the replays the info
    bytes and frame_scale change. Noise std = the rms of the tx samples: the
    hard decisions must hold errors."""
    p = ALL_CONFIGS[name]
    g = O.geometry(p)
    k, bpf, msg, npts = p["mod_type"], g["bytes_per_frame"], g["message_len"], g["npts"]
    nf = persistent_nf() if persistent else 3
    nb = M.fec_max_info_bits(bpf * 8, rate)
    nbytes, nllr = (nb + 7) // 8, npts * k
    wsz = M.fec_workspace_size(nf, nb)
    if name == "N64_k1" and rate == F.R12:
        assert nb == 26
    if name == "D_qpsk":
        assert nb >= 1019 and wsz > 0
    m = modem(name)
    noise = tx_rms(name)
    info = torch.zeros((nf * nbytes,), dtype=torch.uint8, device="cuda")
    fs = torch.ones((nf,), dtype=torch.float64, device="cuda")
    ws = torch.empty((wsz,), dtype=torch.uint8, device="cuda") if wsz else None
    e_hard = torch.zeros((1,), dtype=torch.int64, device="cuda")
    e_dec = torch.zeros((1,), dtype=torch.int64, device="cuda")
    live = {"coded": nf * bpf, "iq": nf * msg, "llr": nf * nllr, "cons": nf * npts, "hard": nf * bpf,
            "dec": nf * nbytes}
    dt = {"coded": torch.uint8, "iq": torch.complex128, "llr": torch.int8, "cons": torch.complex128,
          "hard": torch.uint8, "dec": torch.uint8}
    outs = {n_: out_buf(live[n_], dt[n_]) for n_ in live}
    cases = [(payload(nf * nbytes, 21 + c), np.random.default_rng(3 + c).uniform(0.25, 4.0, nf)) for c in (0, 1)]

    def load_case(c):
        load(info, cases[c][0])
        load(fs, cases[c][1])

    def run():
        m.fec_encode(info, nf, nb, rate, outs["coded"], coded_stride=bpf)
        m.tx(outs["coded"], nf, outs["iq"], noise_std=noise, seed=LINK_SEED)
        m.rx_soft(outs["iq"], nf, outs["llr"], LINK_SCALE, M.LLR_I8, frame_scale=fs, constell_out=outs["cons"],
                  bytes_out=outs["hard"], ref=outs["coded"], bit_errors=e_hard)
        m.fec_decode(outs["llr"], nf, nb, rate, outs["dec"], fmt=M.LLR_I8, llr_stride=nllr, workspace=ws,
                     ref=info, bit_errors=e_dec)

    _, _, r1, r2, counts = replay_protocol(run, load_case, outs, live, counters=(e_hard, e_dec))
    want_hard = want_dec = 0
    for c, r in ((0, r1), (1, r2)):
        what = f"{name} rate {rate} x{nf} replay {c + 1}"
        ibits = F.unpack(cases[c][0].reshape(nf, nbytes), nb)
        coded = np.zeros((nf, bpf), np.uint8)
        packed = F.pack(F.encode(ibits, rate))
        coded[:, :packed.shape[1]] = packed
        assert np.array_equal(r["coded"][:nf * bpf].reshape(nf, bpf), coded), what
        iq = np.ascontiguousarray(r["iq"][:nf * msg])
        clean = O.tx_batch(p, coded.reshape(-1), nf, threads=8)
        noisy = O.awgn(clean, noise, seed=LINK_SEED, threads=8)
        assert rel_err(iq - clean, noisy - clean) < 1e-6  # the channel model's bar on the noise component
        E, hard, _ = O.rx_batch(p, iq, nf, msg, threads=8)
        E = E.reshape(nf, npts)
        cons = r["cons"][:nf * npts].reshape(nf, npts)
        assert rel_err(cons, E) < TOL, what
        assert np.array_equal(r["hard"][:nf * bpf], hard), what
        s_f = LINK_SCALE * cases[c][1]
        llr = r["llr"][:nf * nllr].reshape(nf, npts, k)
        SM.check_i8(llr, SM.ref_llr(k, E, s_f[:, None]), (4.0 * s_f * 1e-9 * np.abs(E).max(axis=1))[:, None, None],
                    what=what + " vs oracle")
        SM.check_i8(llr, SM.ref_llr(k, cons, s_f[:, None]), (s_f * 1e-13)[:, None, None], what=what + " vs own points")
        dbits, _ = F.viterbi(llr.reshape(nf, nllr).astype(np.int64), nb, rate)
        assert np.array_equal(r["dec"][:nf * nbytes].reshape(nf, nbytes), F.pack(dbits)), what
        herr = int(np.unpackbits(hard.reshape(nf, bpf) ^ coded).sum())
        assert herr > 0, "the noise must put errors into the hard decisions"
        want_hard += herr
        want_dec += int((dbits != ibits).sum())
    print(f"{name} rate {rate} x{nf}: hard bit errors {want_hard}, decoded bit errors {want_dec} over two replays")
    assert counts == [want_hard, want_dec]
    # the LLRs followed frame_scale without a re-capture: the two replays' scales differ on every frame
    assert np.all(cases[0][1] != cases[1][1])


# ------------------------------------------------------------------ 2. hard rx, the queue counter
@functools.lru_cache(maxsize=None)
def hard_case(name, nf, c):
    """(payload, noisy samples at 6 dB) of data set c."""
    p = ALL_CONFIGS[name]
    data = payload(nf * O.geometry(p)["bytes_per_frame"], 7 + c)
    x = O.tx_batch(p, data, nf, threads=8)
    iq = O.awgn(x, tx_rms(name) * 10 ** (-6 / 20), seed=11 + c, threads=8)
    return data, iq


@pytest.mark.parametrize("name,mode,persistent", [("N64_k1", "f64", True), ("N64_k1", "i16", True),
                                                  ("D_p16", "f64", False), ("D_s12_staged", "bytes_only", False)])
def test_hard_rx(name, mode, persistent):
    """rx / rx_i16 at persistent size (every workgroup takes frames from the
    per-stream queue counter, which only the previous launch's last workgroup
    re-zeroes), the few-frame wide kernel (D_p16), and the staged geometry
    with bytes_out only (the context's scratch, sized by the eager warm-up).
    After the replays one eager rx on the default stream and one on the
    capture stream: a counter the graph left dirty would show there."""
    p = ALL_CONFIGS[name]
    g = O.geometry(p)
    bpf, msg, npts = g["bytes_per_frame"], g["message_len"], g["npts"]
    nf = persistent_nf() if persistent else 3
    m = modem(name)
    i16 = mode == "i16"
    full = mode != "bytes_only"
    inp = torch.zeros((2 * nf * msg,), dtype=torch.int16, device="cuda") if i16 else \
        torch.zeros((nf * msg,), dtype=torch.complex128, device="cuda")
    ref = torch.zeros((nf * bpf,), dtype=torch.uint8, device="cuda")
    errs = torch.zeros((1,), dtype=torch.int64, device="cuda")
    live = {"bytes": nf * bpf}
    outs = {"bytes": out_buf(nf * bpf, torch.uint8)}
    if full:
        live["cons"] = nf * npts
        outs["cons"] = out_buf(nf * npts, torch.complex128)

    def samples(c):
        """(what the GPU reads, the samples the oracle decodes)."""
        _, iq = hard_case(name, nf, c)
        if not i16:
            return iq, iq
        x16 = O.get_int16(iq, p["mult"])
        w = x16.astype(np.float64)
        return x16, w[0::2] + 1j * w[1::2]

    def load_case(c):
        load(inp, samples(c)[0])
        load(ref, hard_case(name, nf, c)[0])

    def call(o):
        fn = m.rx_i16 if i16 else m.rx
        if full:
            fn(inp, nf, constell_out=o["cons"], bytes_out=o["bytes"], ref=ref, bit_errors=errs)
        else:
            fn(inp, nf, bytes_out=o["bytes"])

    def check(c, r, what):
        ocons, obytes, oerrs = O.rx_batch(p, samples(c)[1], nf, msg, ref=hard_case(name, nf, c)[0], threads=8)
        assert np.array_equal(r["bytes"][:nf * bpf], obytes), what
        if full:
            assert rel_err(r["cons"][:nf * npts], ocons) < TOL, what
        return oerrs

    g_, s, r1, r2, counts = replay_protocol(lambda: call(outs), load_case, outs, live, counters=(errs,) if full else ())
    want = check(0, r1, f"{name} {mode} replay 1") + check(1, r2, f"{name} {mode} replay 2")
    if full:
        assert want > 0 and counts == [want]
    # one more replay, then eager launches with no replay in between them
    g_.replay()
    torch.cuda.synchronize()
    for stream in (torch.cuda.default_stream(), s):
        for t in outs.values():
            fill_sentinel(t)
        torch.cuda.synchronize()  # the capture stream does not wait for the default stream's fills
        with torch.cuda.stream(stream):
            call(outs)
        torch.cuda.synchronize()
        for k_, t in outs.items():
            assert is_sentinel(t[live[k_]:])
        check(1, {k_: host(t) for k_, t in outs.items()}, f"{name} {mode} eager after the replays")


# ------------------------------------------------------------------ 3. sync front end
@pytest.mark.parametrize("fused", [False, True])
def test_sync_front_end(fused):
    """Golden config, 3 impaired frames (test_gpu_sync.py's _impaired_frames).
    The chain works in place, so it starts with a captured ofdm_copy from a
    pristine buffer; then cfo_estimate -> sync_chain -> chan_estimate -> rx
    with the estimated channel, or sync_frames(SYNC_ALL) for the three middle
    calls. Bars: test_batched_sync_chain_matches_oracle's."""
    cfg = G
    m = modem("G")
    g = O.geometry(cfg)
    nf, L, t2, D = 3, g["frame_len"], cfg["t2sin_size"], cfg["num_data_subc"]
    n = g["preamble_len"] + g["message_len"]
    nsym = cfg["num_pr_symb"] + cfg["num_symb"]
    bpf, npts = g["bytes_per_frame"], g["npts"]
    pre, modp, _ = O.preamble_setup(cfg)
    cases = [_impaired_frames(cfg, nf, seed=31 + c) for c in (0, 1)]
    src = torch.zeros((nf * L,), dtype=torch.complex128, device="cuda")
    live = {"x": nf * L, "cfo": nf, "chan": nf * D, "cons": nf * npts, "bytes": nf * bpf}
    dt = {"x": torch.complex128, "cfo": torch.float64, "chan": torch.complex128, "cons": torch.complex128,
          "bytes": torch.uint8}
    outs = {k: out_buf(live[k], dt[k]) for k in live}
    x = outs["x"]
    mwp, message = x[t2:], x[t2 + g["preamble_len"]:]

    def run():
        m.copy(x, src, nf * L * 16)
        if fused:
            m.sync_frames(mwp, nf, L, M.SYNC_ALL, cfo_out=outs["cfo"], chan_out=outs["chan"])
        else:
            m.cfo_estimate(mwp, nf, L, cfg["num_pr_symb"], outs["cfo"])
            m.sync_chain(mwp, nf, L, n, nsym, outs["cfo"])
            m.chan_estimate(mwp, nf, L, outs["chan"])
        m.rx(message, nf, frame_stride=L, chan=outs["chan"], chan_stride=D, constell_out=outs["cons"],
             bytes_out=outs["bytes"])

    _, _, r1, r2, _ = replay_protocol(run, lambda c: load(src, cases[c][0]), outs, live)
    for c, r in ((0, r1), (1, r2)):
        stream = cases[c][0]
        for f in range(nf):
            assert np.array_equal(r["x"][f * L: f * L + t2], stream[f * L: f * L + t2])  # the T2 part: copied only
            rr = stream[f * L + t2: f * L + L].copy()
            cf = O.pilot_freq_sinh(cfg, rr[:g["preamble_len"]])
            assert r["cfo"][f] == cf
            rr = O.pr_phase_sinh(O.cp_freq_sinh(cfg, O.freq_shift(rr, cf)), pre)
            assert rel_err(r["x"][f * L + t2: f * L + L], rr) < TOL_SYNC
            ch = O.chan_char_lq(cfg, rr[:g["preamble_len"]], modp)
            assert rel_err(r["chan"][f * D:(f + 1) * D], ch) < TOL_SYNC
            oc = O.ofdm_fft(cfg, rr[g["preamble_len"]:]) / np.tile(ch, cfg["num_symb"])
            ob, _ = O.demod(cfg["mod_type"], oc)
            assert rel_err(r["cons"][f * npts:(f + 1) * npts], oc) < TOL_SYNC
            assert np.array_equal(r["bytes"][f * bpf:(f + 1) * bpf], ob)
            assert np.array_equal(ob, cases[c][1][f * bpf:(f + 1) * bpf])  # and the frame decodes


# ------------------------------------------------------------------ 4. detectors
def test_detectors_on_the_golden_capture():
    """t2_scan (rel_out and first_out through the context's scratch),
    find_preamble in the split form (6 starts: per-start completion counters)
    and in the one-workgroup form (100 starts), one graph on the golden
    capture. t2_scan's start is a host argument and stays; between the
    replays the samples shift (the buffer is overwritten with x[s:], zeros
    behind) and the start indices change."""
    m = modem("G")
    x0 = golden()["data"]
    n, t2 = len(x0), G["t2sin_size"]
    pb = int(golden()["preamble_begin"][0]) - 1
    start, shift = 5000, 4321
    nblk = (n - start) // t2
    rng = np.random.default_rng(5)
    xs = [x0, np.concatenate([x0[shift:], np.zeros(shift, np.complex128)])]
    few = [np.array([10752, 10752 + 256, 0, 19000, 30000, n - 100], np.int32),
           np.array([pb - shift - 300, 19000 - shift, n - 50, 7, pb - shift, 12345], np.int32)]
    many = [np.concatenate([[pb - 300 - s, pb - 1 - s, pb - s, pb + 1 - s, 10752 - s, 19000 - s],
                            rng.integers(0, n - 1, 94)]).astype(np.int32) for s in (0, shift)]
    dx = torch.zeros((n,), dtype=torch.complex128, device="cuda")
    d_few = torch.zeros((6,), dtype=torch.int32, device="cuda")
    d_many = torch.zeros((100,), dtype=torch.int32, device="cuda")
    live = {"rel": nblk, "first": 1, "few": 6, "many": 100}
    dt = {"rel": torch.float64, "first": torch.int32, "few": torch.int32, "many": torch.int32}
    outs = {k: out_buf(live[k], dt[k]) for k in live}

    def load_case(c):
        load(dx, xs[c])
        load(d_few, few[c])
        load(d_many, many[c])

    def run():
        m.t2_scan(dx, n, start, rel_out=outs["rel"], first_out=outs["first"])
        m.find_preamble(dx, n, d_few, 6, outs["few"])
        m.find_preamble(dx, n, d_many, 100, outs["many"])

    _, _, r1, r2, _ = replay_protocol(run, load_case, outs, live)
    firsts = []
    for c, r in ((0, r1), (1, r2)):
        assert np.abs(r["rel"][:nblk] - O.t2_corr(G, xs[c][start:])).max() < 1e-12
        firsts.append(O.find_t2sin(G, xs[c], start))
        assert int(r["first"][0]) == firsts[-1]
        assert list(r["few"][:6]) == [O.find_preamble(G, xs[c], int(s)) for s in few[c]]
        assert list(r["many"][:100]) == [O.find_preamble(G, xs[c], int(s)) for s in many[c]]
        assert (r["many"][:6] >= 0).all(), "the starts around the preamble must find it"
    assert firsts[0] >= 0 and firsts[1] >= 0 and firsts[0] != firsts[1]


# ------------------------------------------------------------------ 5. the flat kernels in one graph
def _fft_write_ref(cfg, pts, nf):
    N, D, P, S = cfg["fft_size"], cfg["num_data_subc"], cfg["num_pilot_subc"], cfg["num_symb"]
    out = np.zeros(nf * N * S, np.complex128)
    for f in range(nf):
        o = np.zeros(N * S, np.complex128)
        O.lib().orc_fft_write(N, D, P, S, cfg["pilot_ampl"] / 1000, O._d(pts[f * D * S:(f + 1) * D * S].copy()), O._d(o))
        out[f * N * S:(f + 1) * N * S] = o
    return out


def _fft_read_ref(cfg, fb, nf):
    N, D, P, S = cfg["fft_size"], cfg["num_data_subc"], cfg["num_pilot_subc"], cfg["num_symb"]
    out = np.zeros(nf * D * S, np.complex128)
    for f in range(nf):
        o = np.zeros(D * S, np.complex128)
        O.lib().orc_fft_read(N, D, P, S, cfg["pilot_ampl"] / 1000, O._d(fb[f * N * S:(f + 1) * N * S].copy()), O._d(o))
        out[f * D * S:(f + 1) * D * S] = o
    return out


@pytest.mark.parametrize("name", ["D", "D_qam64"])
def test_flat_kernels_in_one_graph(name):
    """map, bit_convert, demap (behind a captured copy: it clamps in place),
    soft_demap, fft_write, fft_read, int16_to_double, double_to_int16, tx_frames and
    rx_read as one linear graph; references and bars of the eager tests in
    test_gpu_parity.py and test_gpu_soft.py."""
    cfg = ALL_CONFIGS[name]
    m = modem(name)
    g = O.geometry(cfg)
    k, N, D, S = cfg["mod_type"], cfg["fft_size"], cfg["num_data_subc"], cfg["num_symb"]
    nf, bpf, msg, npts, flen = 2, g["bytes_per_frame"], g["message_len"], g["npts"], g["frame_len"]
    nmap, npt, n16, scale = 333, 1000 + k, 4099, 2.0
    nmapped = (nmap * 8 + k - 1) // k
    ndemap = (npt * k + 7) // 8

    def case(c):
        rng = np.random.default_rng(100 * c + k)
        d = {"data": payload(nmap, seed=k + c)}
        pts = (rng.standard_normal(npt) + 1j * rng.standard_normal(npt)) * 0.8
        pts[:3] = [0.0, 1.0 / 3.0 + 1j, -3.0 - 3j]
        d["pts"] = pts
        d["fpts"] = O.constellation(k)[rng.integers(0, 1 << k, nf * D * S)]
        d["fb"] = O.awgn(_fft_write_ref(cfg, d["fpts"], nf), 0.05, seed=3 + c)
        d["v16"] = rng.integers(-32768, 32767, 2 * n16, dtype=np.int16)
        d["xd"] = rng.uniform(-150.0, 150.0, n16) + 1j * rng.uniform(-150.0, 150.0, n16)  # |x * mult| < 32767
        d["fbytes"] = payload(nf * bpf, seed=40 + c)
        d["iq"] = O.awgn(O.tx_batch(cfg, payload(nf * bpf, seed=50 + c), nf), 0.05, seed=22 + c)
        d["chan"] = np.exp(1j * rng.uniform(-0.3, 0.3, nf * D)) * rng.uniform(0.8, 1.2, nf * D)
        return d

    cases = [case(0), case(1)]
    ins = {k_: dev(v) for k_, v in cases[0].items()}
    live = {"mapped": nmapped, "work": npt, "dbytes": ndemap, "llr": npt * k, "fbuf": nf * N * S, "rest": nf * D * S,
            "dbl": n16, "i16": 2 * n16, "frames": nf * flen, "frames16": 2 * nf * flen, "read": nf * npts,
            "cons": nf * npts, "rbytes": nf * bpf, "regroup": (nmap * 8 + 5) // 6}
    c128 = torch.complex128
    dt = {"mapped": c128, "work": c128, "dbytes": torch.uint8, "llr": torch.float32, "fbuf": c128, "rest": c128,
          "dbl": c128, "i16": torch.int16, "frames": c128, "frames16": torch.int16, "read": c128, "cons": c128,
          "rbytes": torch.uint8, "regroup": torch.uint8}
    outs = {k_: out_buf(live[k_], dt[k_]) for k_ in live}

    def load_case(c):
        for k_, v in cases[c].items():
            load(ins[k_], v)

    def run():
        m.map(ins["data"], nmap, outs["mapped"])
        assert m.bit_convert(ins["data"], nmap, 8, 6, outs["regroup"]) == live["regroup"]
        m.copy(outs["work"], ins["pts"], npt * 16)
        m.demap(outs["work"], npt, outs["dbytes"])
        m.soft_demap(ins["pts"], npt, outs["llr"], scale, M.LLR_F32)
        m.fft_write(ins["fpts"], nf, outs["fbuf"])
        m.fft_read(ins["fb"], nf, outs["rest"])
        m.int16_to_double(ins["v16"], n16, outs["dbl"])
        m.double_to_int16(ins["xd"], n16, outs["i16"])
        m.tx_frames(ins["fbytes"], nf, outs["frames"], outs["frames16"])
        m.rx_read(ins["iq"], nf, ins["chan"], outs["read"], chan_stride=D, constell_out=outs["cons"],
                  bytes_out=outs["rbytes"])

    _, _, r1, r2, _ = replay_protocol(run, load_case, outs, live)
    for k_, v in cases[1].items():
        assert np.array_equal(host(ins[k_]).view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), f"input {k_} modified"
    for c, r in ((0, r1), (1, r2)):
        d = cases[c]
        assert np.array_equal(r["mapped"][:nmapped], O.mod(k, d["data"]))
        assert np.array_equal(r["regroup"][:live["regroup"]], O.bit_convert(6, 8, d["data"]))
        ob, opts = O.demod(k, d["pts"])
        assert np.array_equal(r["dbytes"][:ndemap], ob)
        assert np.array_equal(r["work"][:npt], opts)
        SM.check_f32(r["llr"][:npt * k], SM.ref_llr(k, d["pts"], scale).reshape(-1), scale * 1e-13, f"{name} flat")
        assert rel_err(r["fbuf"][:nf * N * S], _fft_write_ref(cfg, d["fpts"], nf)) < TOL
        assert rel_err(r["rest"][:nf * D * S], _fft_read_ref(cfg, d["fb"], nf)) < TOL
        h = r["dbl"][:n16]
        assert np.array_equal(h.real, d["v16"][0::2].astype(np.float64))
        assert np.array_equal(h.imag, d["v16"][1::2].astype(np.float64))
        assert np.array_equal(r["i16"][:2 * n16], O.get_int16(d["xd"], cfg["mult"]))
        want = np.concatenate([O.frame_write(cfg, d["fbytes"][f * bpf:(f + 1) * bpf]) for f in range(nf)])
        assert rel_err(r["frames"][:nf * flen], want) < TOL
        assert_int16_match(r["frames16"][:2 * nf * flen], want, cfg["mult"])
        ocons, _, _ = O.rx_batch(cfg, d["iq"], nf, msg)
        assert rel_err(r["read"][:nf * npts], ocons) < TOL
        read = r["read"][:nf * npts].reshape(nf, npts)
        cons = r["cons"][:nf * npts].reshape(nf, npts)
        div = smith_div(read, np.tile(d["chan"].reshape(nf, D), (1, npts // D)))
        assert rel_err(cons, div) < 1e-14  # test_rx_demod_read_...'s bar for the division
        for f in range(nf):
            assert np.array_equal(r["rbytes"][f * bpf:(f + 1) * bpf], O.demod(k, cons[f])[0])


# ------------------------------------------------------------------ 6. what a capture refuses
def test_first_calls_that_allocate_are_refused_inside_a_capture():
    """The documented exceptions, on contexts that have not made the call
    before: staged rx without constell_out (the scratch), sync_frames without
    cfo_out (the CFO scratch), a new CFO form length (its tables) and
    ofdm_preamble_corr (synchronises). On a capturing stream each returns
    OFDM_ERR_UNSUPPORTED before anything is issued: the capture stays valid,
    the calls around them replay, and nothing was written. After one eager
    call each the first three capture and replay bit for bit."""
    ps = ALL_CONFIGS["D_s12_staged"]
    gs, gg = O.geometry(ps), O.geometry(G)
    ms, mg = M.Modem(ps, 0), M.Modem(G, 0)
    nf, L, t2, D = 3, gg["frame_len"], G["t2sin_size"], G["num_data_subc"]
    iq = dev(hard_case("D_s12_staged", nf, 0)[1])
    stream = _impaired_frames(G, nf, seed=31)[0]
    src = dev(stream)
    cycles = 2 * t2 + G["pr_sin_len"]
    live = {"bytes": nf * gs["bytes_per_frame"], "x": nf * L, "chan": nf * D, "cfo": nf, "cor": cycles, "copy": nf * L}
    dt = {"bytes": torch.uint8, "x": torch.complex128, "chan": torch.complex128, "cfo": torch.float64,
          "cor": torch.float64, "copy": torch.complex128}
    outs = {k: out_buf(live[k], dt[k]) for k in live}
    x = outs["x"]
    calls = {
        "staged rx": lambda: ms.rx(iq, nf, bytes_out=outs["bytes"]),
        "sync_frames": lambda: mg.sync_frames(x[t2:], nf, L, M.SYNC_ALL, chan_out=outs["chan"]),
        "cfo_estimate": lambda: mg.cfo_estimate(x[t2:], nf, L, G["num_pr_symb"], outs["cfo"]),
        "preamble_corr": lambda: mg.preamble_corr(src, nf * L, 0, outs["cor"]),
    }
    for t in outs.values():
        fill_sentinel(t)
    mg.copy(x, src, nf * L * 16)  # (module load of the copy kernel)
    g1, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g1, stream=s):
        mg.copy(x, src, nf * L * 16)
        for what, call in calls.items():
            with pytest.raises(M.OfdmError) as e:
                call()
            assert e.value.code == -2, what  # OFDM_ERR_UNSUPPORTED
        mg.copy(outs["copy"], x, nf * L * 16)
    fill_sentinel(x)
    g1.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(x[:nf * L]), bits(src)) and torch.equal(bits(outs["copy"][:nf * L]), bits(src))
    for k in ("bytes", "chan", "cfo", "cor"):
        assert is_sentinel(outs[k]), f"a refused call wrote {k}"
    # the same calls once eagerly; then they capture
    for what in ("staged rx", "sync_frames", "cfo_estimate"):
        calls[what]()
    torch.cuda.synchronize()
    eager = {k: outs[k].clone() for k in ("bytes", "x", "chan", "cfo")}
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=s):
        mg.copy(x, src, nf * L * 16)
        for what in ("staged rx", "sync_frames", "cfo_estimate"):
            calls[what]()
    for k in eager:
        fill_sentinel(outs[k])
    g2.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(bits(outs[k]), bits(v)), k
        assert is_sentinel(outs[k][live[k]:]) and not is_sentinel(outs[k][:live[k]])
    _, obytes, _ = O.rx_batch(ps, hard_case("D_s12_staged", nf, 0)[1], nf, gs["message_len"])
    assert np.array_equal(host(outs["bytes"])[:live["bytes"]], obytes)
    ms.close()
    mg.close()
