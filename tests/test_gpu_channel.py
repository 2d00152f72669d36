"""The rx sync chain on non-flat channels (tests/common.py CHANNEL_CASES:
multipath, and regions cut a few samples early), where chan_char_lq's unwrap
adjusts tens to hundreds of entries per frame, visits all three states and
changes state up to 75 times in a frame; on the flat, exactly cut frames of
test_gpu_sync.py it adjusts none. Stage by stage and fused, against the
oracle's stages on the same samples, at test_batched_sync_chain_matches_oracle's
bars: CFO equal, samples and channel vector 1e-9 relative, constellation
1e-9, bytes equal. tests/test_channel_cases.py shows on the CPU that every
case is well conditioned at those bars (no compare within 1e-6 rad of +-pi,
no point within 1e-7 of a decision edge)."""
import numpy as np
import pytest

import oracle as O
from common import B, CC, CHAN_ONLY_CASES, CHANNEL_CASES, D, G, TAPS_ECHO, TAPS_FLAT, TAPS_NOTCH, channel_frames, rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

_m = {}


def modem(cfg):
    key = repr(sorted(cfg.items()))
    if key not in _m:
        _m[key] = M.Modem(cfg, 0)
    return _m[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _oracle_stages(cfg, region):
    """main.cpp:60-65 stage by stage on one region."""
    g = O.geometry(cfg)
    pre, modp, _ = O.preamble_setup(cfg)
    cfo = O.pilot_freq_sinh(cfg, region[: g["preamble_len"]])
    shifted = O.freq_shift(region, cfo)
    cp = O.cp_freq_sinh(cfg, shifted)
    ph = O.pr_phase_sinh(cp, pre)
    chan = O.chan_char_lq(cfg, ph[: g["preamble_len"]], modp)
    return cfo, shifted, cp, ph, chan


def _cfo_form_supported(cfg):
    """ofdm_cfo_estimate takes a pilot_freq_sinh form of 2^a or 5 * 2^a points
    with 2^a >= 64; N64_k1 (80 = 5 * 16) and N128_k4_s3 (144) have neither.
    There the GPU stages after it run on the oracle's CFO."""
    L = (cfg["fft_size"] + cfg["cp_size"]) * cfg["num_pr_symb"]
    a = L // 5 if L % 5 == 0 else L
    return a >= 64 and a & (a - 1) == 0


def _stagewise(cfg, regions):
    """cfo_estimate, freq_shift, cp_sync, phase_sync, chan_estimate one by one
    on a batch at stride n, each stage's state against the oracle's."""
    m = modem(cfg)
    nf, n = regions.shape
    D = cfg["num_data_subc"]
    nsym = cfg["num_pr_symb"] + cfg["num_symb"]
    x = dev(regions.reshape(-1))
    cfo = torch.zeros((nf,), dtype=torch.float64, device="cuda")
    chan = torch.zeros((nf * D,), dtype=torch.complex128, device="cuda")
    want = [_oracle_stages(cfg, r) for r in regions]
    if _cfo_form_supported(cfg):
        m.cfo_estimate(x, nf, n, cfg["num_pr_symb"], cfo)
        hcfo = host(cfo)
        for f in range(nf):
            assert hcfo[f] == want[f][0], f
    else:
        with pytest.raises(M.OfdmError, match="form length"):
            m.cfo_estimate(x, nf, n, cfg["num_pr_symb"], cfo)
        cfo = dev(np.array([w[0] for w in want]))
    for k, step in enumerate((lambda: m.freq_shift(x, nf, n, n, cfo), lambda: m.cp_sync(x, nf, n, nsym),
                              lambda: m.phase_sync(x, nf, n, n))):
        step()
        hx = host(x).reshape(nf, n)
        for f in range(nf):
            assert rel_err(hx[f], want[f][1 + k]) < 1e-9, (k, f)
    m.chan_estimate(x, nf, n, chan)
    hchan = host(chan).reshape(nf, D)
    for f in range(nf):
        assert rel_err(hchan[f], want[f][4]) < 1e-9, f
    return want


@pytest.mark.parametrize("case", CHANNEL_CASES, ids=[c[0] for c in CHANNEL_CASES])
def test_sync_stages_and_fused_sync_match_oracle_on_channel_frames(case):
    """Stage by stage, then sync_frames(SYNC_ALL) + rx, per frame against the
    oracle. chan_kernel's unwrap_scan<T> runs with T = N/8 threads: 8
    (N64_k1), 16, 64 (D), 128, 256 (B: four wave totals) and 512 (C: eight).
    The two smallest geometries have no GPU CFO estimate (_cfo_form_supported):
    their later stages, fused and one by one, take the oracle's CFO."""
    name, cfg, taps, offset, seed, nf = case
    m = modem(cfg)
    g = O.geometry(cfg)
    D, npre = cfg["num_data_subc"], g["preamble_len"]
    regions, _ = channel_frames(cfg, nf, seed, taps, offset)
    n = regions.shape[1]
    want = _stagewise(cfg, regions)
    x = dev(regions.reshape(-1))
    cfo = torch.zeros((nf,), dtype=torch.float64, device="cuda")
    chan = torch.zeros((nf * D,), dtype=torch.complex128, device="cuda")
    if _cfo_form_supported(cfg):
        m.sync_frames(x, nf, n, M.SYNC_ALL, cfo_out=cfo, chan_out=chan)
    else:
        cfo = dev(np.array([w[0] for w in want]))
        m.sync_frames(x, nf, n, M.SYNC_ALL & ~M.SYNC_CFO, cfo_in=cfo, chan_out=chan)
    out = torch.zeros((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
    cons = torch.zeros((nf * g["npts"],), dtype=torch.complex128, device="cuda")
    m.rx(x[npre:], nf, frame_stride=n, chan=chan, chan_stride=D, constell_out=cons, bytes_out=out)
    hcfo, hchan, hx = host(cfo), host(chan).reshape(nf, D), host(x).reshape(nf, n)
    hcons, hout = host(cons).reshape(nf, -1), host(out).reshape(nf, -1)
    for f in range(nf):
        c, _, _, r, ch = want[f]
        assert hcfo[f] == c
        assert rel_err(hx[f], r) < 1e-9
        assert rel_err(hchan[f], ch) < 1e-9
        oc = O.ofdm_fft(cfg, r[npre:]) / np.tile(ch, cfg["num_symb"])
        ob, _ = O.demod(cfg["mod_type"], oc)
        assert rel_err(hcons[f], oc) < 1e-9
        assert np.array_equal(hout[f], ob)


@pytest.mark.parametrize("case", CHAN_ONLY_CASES, ids=[c[0] for c in CHAN_ONLY_CASES])
def test_chan_estimate_three_and_four_entries_per_thread(case):
    """N = 512 with 384 and 448 data carriers: half = 192 and 224 over
    chan_kernel's 64 threads, so unwrap_scan<64> holds R = 3 and R = 4 entries
    per thread (every other geometry here has R <= 2). rx refuses D > N/2, so
    the stages, the synced samples and the channel vector are compared."""
    name, cfg, taps, offset, seed, nf = case
    T = cfg["fft_size"] // 8
    assert (cfg["num_data_subc"] // 2 - 1 + T - 1) // T == (3 if cfg["num_data_subc"] == 384 else 4)
    regions, _ = channel_frames(cfg, nf, seed, taps, offset)
    _stagewise(cfg, regions)


# bit-for-bit comparisons of two GPU paths: no conditioning needed, so G (not
# in the case table) stands beside D, B and C
CHAIN_CASES = [("G-notch-o17", G, TAPS_NOTCH, 17, 45, 3), ("D-echo-o64", D, TAPS_ECHO, 64, 35, 3),
               ("B-flat-ocp2", B, TAPS_FLAT, B["cp_size"] // 2, 37, 3), ("C-echo-o17", CC, TAPS_ECHO, 17, 39, 3)]


@pytest.mark.parametrize("case", CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_sync_chain_one_launch_equals_stagewise_on_channel_frames(case):
    """ofdm_sync_chain (freq_shift + cp_sync + phase_sync in one launch) equals
    the three single-stage launches bit for bit on non-flat frames too, in
    place and in each stage copy."""
    name, cfg, taps, offset, seed, nf = case
    m = modem(cfg)
    regions, _ = channel_frames(cfg, nf, seed, taps, offset)
    n = regions.shape[1]
    nsym = cfg["num_pr_symb"] + cfg["num_symb"]
    x0 = dev(regions.reshape(-1))
    cfo = torch.zeros((nf,), dtype=torch.float64, device="cuda")
    m.cfo_estimate(x0, nf, n, cfg["num_pr_symb"], cfo)
    ref = x0.clone()
    states = []
    for step in (lambda: m.freq_shift(ref, nf, n, n, cfo), lambda: m.cp_sync(ref, nf, n, nsym),
                 lambda: m.phase_sync(ref, nf, n, n)):
        step()
        states.append(ref.clone())
    x = x0.clone()
    outs = [torch.full((nf * n,), np.nan, dtype=torch.complex128, device="cuda") for _ in range(3)]
    m.sync_chain(x, nf, n, n, nsym, cfo, *outs, out_stride=n)
    torch.cuda.synchronize()
    assert torch.equal(x, ref)
    for k in range(3):
        assert torch.equal(outs[k], states[k]), k
