"""tx's dead groups (ofdm_tx_sparse): a wave whose 64 bins of a register group
all lie in the guard band skips that group's mapping and prunes its first
butterfly. Every shape that reaches another path of the tx kernel is checked
against the oracle at test_gpu_parity's tolerances (1e-10 relative noise-free,
1e-6 relative on the noise component), and, where the switch applies, with the
skipping on against off (the kernel's earlier mapping and full butterfly) with
torch.equal: f64 samples, int16 wire samples, and FFT_FORM::write on points.
The mask table is checked against a brute-force count over the per-bin codes."""
import numpy as np
import pytest

import oracle as O
from common import B, CC, D, assert_int16_match, cfg, payload, rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

TOL, TOL_NOISE = 1e-10, 1e-6
D480 = cfg(D, num_data_subc=480, num_pilot_subc=16)
N256 = cfg(D, fft_size=256, num_data_subc=128, num_pilot_subc=8, cp_size=64, mod_type=2)
# name: (config, frames, masks the layout gives, what the shape reaches)
SHAPES = {
    "D": (D, 2, [0x18], "one-wave kernel"),
    "B": (B, 2, [0x38, 0x3c, 0x3c, 0x1c], "dead and partly dead groups in one workgroup, both pruned forms"),
    "C": (CC, 1, [0x38] + [0x3c] * 6 + [0x1c], "T = 512; masks that contain a pruned form's pattern"),
    "D480": (D480, 2, [0], "no whole group is zero: masks 0, the general path"),
    "N256": (N256, 2, [], "T < 64: no masks"),
    "D_cp100": (cfg(D, cp_size=100), 2, [0x18], "general CP path"),
    "D_s7_600": (cfg(D, num_symb=7), 600, [0x18], "more symbols than the 4096-workgroup grid, S not dividing it"),
}
_modems = {}


def modem(name):
    if name not in _modems:
        _modems[name] = M.Modem(SHAPES[name][0], 0)
    return _modems[name]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def both_ways(m, run):
    """run() with the skipping on, and off where the switch applies: the two
    outputs must be equal; returns the skipping-on outputs."""
    active = m.tx_sparse(True)
    on = run()
    if active:
        assert m.tx_sparse(False) is False
        off = run()
        assert m.tx_sparse(True) is True
        torch.cuda.synchronize()
        for a, b in zip(on, off):
            assert torch.equal(a, b)
    return on


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mask_table_matches_brute_force(name):
    c, _, want, _ = SHAPES[name]
    m = modem(name)
    masks, codes = m.tx_dead_tables()
    N = c["fft_size"]
    T = N // 8
    zero = 257 << 21
    brute = []
    for w in range(T // 64):
        bits = 0
        for i in range(8):
            if sum(int(codes[64 * w + lane + T * i] == zero) for lane in range(64)) == 64:
                bits |= 1 << i
        brute.append(bits)
    assert list(masks) == brute == want
    # the codes name the layout's unused bins and no others
    used = np.zeros(N, bool)
    seg = c["num_data_subc"] // c["num_pilot_subc"]
    g = m.geo
    for j in range(c["num_pilot_subc"]):
        used[g.pilot_bin[j]] = True
        used[g.segment_bin[j]:g.segment_bin[j] + seg] = True
    assert np.array_equal(codes == zero, ~used)
    assert m.tx_sparse() == any(want)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tx_f64_and_int16_match_oracle_and_switch(name):
    c, nf, _, _ = SHAPES[name]
    m = modem(name)
    g = O.geometry(c)
    data = dev(payload(nf * g["bytes_per_frame"], seed=41))

    def run():
        iq = torch.zeros((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
        iq16 = torch.zeros((2 * nf * g["message_len"],), dtype=torch.int16, device="cuda")
        only = torch.zeros_like(iq)
        m.tx(data, nf, iq, iq16_out=iq16)
        m.tx(data, nf, only)  # the f64-only instantiation
        return iq, iq16, only

    iq, iq16, only = both_ways(m, run)
    ref = O.tx_batch(c, host(data), nf)
    err = rel_err(host(iq), ref)
    print(name, "tx rel err", err)
    assert err < TOL
    assert torch.equal(iq, only)
    assert_int16_match(host(iq16), ref, c["mult"])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fft_write_points_match_oracle_and_switch(name):
    c, nf, _, _ = SHAPES[name]
    nf = min(nf, 3)
    m = modem(name)
    N, Dn, P, S = c["fft_size"], c["num_data_subc"], c["num_pilot_subc"], c["num_symb"]
    rng = np.random.default_rng(5)
    pts = O.constellation(c["mod_type"])[rng.integers(0, 1 << c["mod_type"], nf * Dn * S)]
    d_pts = dev(pts)

    def run():
        fb = torch.zeros((nf * N * S,), dtype=torch.complex128, device="cuda")
        m.fft_write(d_pts, nf, fb)
        return (fb,)

    (fb,) = both_ways(m, run)
    want = []
    for f in range(nf):
        o = np.zeros(N * S, np.complex128)
        O.lib().orc_fft_write(N, Dn, P, S, c["pilot_ampl"] / 1000, O._d(pts[f * Dn * S:(f + 1) * Dn * S].copy()), O._d(o))
        want.append(o)
    assert rel_err(host(fb), np.concatenate(want)) < TOL


# the 2^32 wrap of the sample counter on the first sample of frame 0's symbol
# 3, on its last sample, inside it, and in no symbol: sample_offset for symbols
# of L samples
WRAPS = {"first": lambda L: (1 << 32) - 3 * L, "last": lambda L: (1 << 32) - 3 * L - (L - 1),
         "middle": lambda L: (1 << 32) - 3 * L - 300, "none": lambda L: 0}


@pytest.mark.parametrize("where", sorted(WRAPS))
@pytest.mark.parametrize("name", ["D", "B"])
def test_tx_awgn_matches_oracle_and_switch(name, where):
    c, nf, _, _ = SHAPES[name]
    m = modem(name)
    g = O.geometry(c)
    L = c["fft_size"] + c["cp_size"]
    off = WRAPS[where](L)
    host_data = payload(nf * g["bytes_per_frame"], seed=43)
    data = dev(host_data)
    seed = (9 << 40) + 4321

    def run():
        iq = torch.zeros((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
        both = torch.zeros_like(iq)
        iq16 = torch.zeros((2 * nf * g["message_len"],), dtype=torch.int16, device="cuda")
        m.tx(data, nf, iq, noise_std=0.3, seed=seed, sample_offset=off)
        m.tx(data, nf, both, iq16_out=iq16, noise_std=0.3, seed=seed, sample_offset=off)
        return iq, both, iq16

    iq, both, iq16 = both_ways(m, run)
    clean = O.tx_batch(c, host_data, nf)
    want = O.awgn(clean, 0.3, seed=seed, sample_offset=off)
    if where != "none":  # the wrap is where the case says
        first = (1 << 32) - off
        assert {"first": first % L == 0, "last": first % L == L - 1, "middle": 0 < first % L < L - 1}[where]
        assert first // L == 3
    for got in (host(iq), host(both)):
        err = rel_err(got - clean, want - clean)
        print(name, where, "noise rel err", err)
        assert err < TOL_NOISE
    assert_int16_match(host(iq16), clean, c["mult"])  # the wire samples carry no noise
