"""The stand-alone sync detectors on every kernel instance and edge:
ofdm_t2_scan, ofdm_find_preamble, ofdm_preamble_corr and ofdm_cfo_estimate on
the cases of tests/detector_cases.py (checked on the CPU by
tests/test_detector_cases.py). The stream walker has its own T2 and preamble
search, so no stream test runs these kernels. Every expected value is the
oracle's; every output carries sentinels past its end; inputs are checked
unmodified.

- t2_scan_kernel<LOGN>: all seven sizes (64 .. 4096: 32, 16, 8, 4, 2, 1, 1
  blocks per workgroup, the three reduce paths), mask bands clipped at 0 and
  at size - 1 and overlapping, starts on and off the block grid, block counts
  that leave dead groups, no block at all, blocks of zeros / with a NaN / with
  an Inf, the crafted near-level blocks of tests/t2_level_cases.py.
  rel_out within 1e-12 of the oracle's (the golden test's bar). Measured on
  the MI355X: 5.6e-16 at size 64 rising to 3.3e-15 at 4096, the largest of
  all cases.
- find_preamble_kernel: pr_sin_len 8 .. 640 (the tails of the correlation and
  the energy loops), 136 .. 4736 lags (1 .. 19 slices, 162,640 bytes of LDS at
  the most), both launch forms, three stream textures, negative starts,
  windows past n, n below the buffer, and first passing lags with a ratio of
  level (1 +- d), d down to 1e-13.
  preamble_corr agrees with the serial FP64 reference at rel_err < 1e-10
  (test_preamble_corr's bar). Measured on the MI355X: 5.6e-16 at the most
  (pr_sin_len 257), 3.3e-16 .. 4.5e-16 at the other shapes.
- cfo_kernel<LOGM, G>: all twelve instances and five multi-symbol forms,
  exact-tie frames included, bitwise.
- The status codes of the calls that cannot run."""
import functools

import numpy as np
import pytest

import detector_cases as DC
import oracle as O
import t2_level_cases as T
from common import rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ofdm_mi355x as M  # noqa: E402

PAD = 64
SENT = 77
ERR_INVALID, ERR_UNSUPPORTED = -1, -2
_m = {}


def modem(cfg):
    key = repr(sorted(cfg.items()))
    if key not in _m:
        _m[key] = M.Modem(cfg, 0)
    return _m[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    """About thirty configs get a context here: released when the module is done."""
    yield
    for m in _m.values():
        m.close()
    _m.clear()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the fixtures are read-only)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def unmodified(d_x, x):
    """Bit for bit (the T2 streams hold a NaN)."""
    return np.array_equal(host(d_x).view(np.int64), np.ascontiguousarray(x).view(np.int64))


def f64_out(n):
    return torch.full((n + PAD,), 9.0, dtype=torch.float64, device="cuda")


def i32_out(n):
    return torch.full((n + PAD,), SENT, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------ ofdm_t2_scan
def run_t2_scan(m, d_x, n, start, nb):
    """(first, rel) of one scan, the sentinels past both checked."""
    rel, first = f64_out(nb), i32_out(1)
    m.t2_scan(d_x, n, start, rel_out=rel, first_out=first)
    h_rel, h_first = host(rel), host(first)
    assert np.all(h_rel[nb:] == 9.0) and np.all(h_first[1:] == SENT), "written past the range"
    return int(h_first[0]), h_rel[:nb]


def check_rel(got, want, what):
    assert np.array_equal(got != 0, want != 0), what
    err = float(np.abs(got - want).max()) if len(want) else 0.0
    assert err < 1e-12, (what, err)
    return err


@pytest.mark.parametrize("key", list(DC.T2_CONFIGS))
def test_t2_scan(key):
    c = DC.t2_case(key)
    m = modem(c["cfg"])
    d_x = {name: dev(x) for name, x in c["streams"].items()}
    worst, answers = 0.0, {}
    for scan in c["scans"]:
        tag, name, n, start = scan
        want_first, want_rel = DC.t2_want(key, scan)
        first, rel = run_t2_scan(m, d_x[name], n, start, len(want_rel))
        assert first == want_first, (key, tag, first, want_first)
        if n - start < c["cfg"]["t2sin_size"]:
            assert first == -1 and len(rel) == 0  # no block: rel_out is all sentinel (checked above)
        worst = max(worst, check_rel(rel, want_rel, (key, tag)))
        answers[tag] = want_first
    # back to back, no synchronisation between: each launch leaves the scratch as the next needs it
    order = ("plain-0", "plain-late", "plain-mid", "no-block-0", "plain-1", "plain-late")
    assert len({answers[t] for t in order}) >= 3
    outs = [i32_out(1) for _ in order]
    scans = {s[0]: s for s in c["scans"]}
    for tag, out in zip(order, outs):
        _, name, n, start = scans[tag]
        m.t2_scan(d_x[name], n, start, first_out=out)
    for tag, out in zip(order, outs):
        h = host(out)
        assert int(h[0]) == answers[tag] and np.all(h[1:] == SENT), (key, tag)
    for name, x in c["streams"].items():
        assert unmodified(d_x[name], x), "the input was modified"
    print(f"t2_scan {key}: max |rel_out - oracle| {worst:.3e}")


@pytest.mark.parametrize("key", list(T.CONFIGS))
def test_t2_scan_decides_the_crafted_near_level_blocks(key):
    """The streams of tests/t2_level_cases.py: one block with a ratio of
    level + delta, |delta| from 1e-5, before the first frame. The scan from 0
    reports the block when delta > 0 and the first frame's marker when not."""
    cfg = T.CONFIGS[key][0]
    m = modem(cfg)
    size = cfg["t2sin_size"]
    worst = 0.0
    for c in T.cases(key):
        x = c["x"]
        want_first, want_rel = O.find_t2sin(cfg, x, 0), O.t2_corr(cfg, x)
        assert (want_first == c["slot"] * size) == (c["delta"] > 0) and want_first >= c["slot"] * size
        first, rel = run_t2_scan(m, dev(x), len(x), 0, len(want_rel))
        assert first == want_first, (key, c["pair"], c["delta"], first, want_first)
        worst = max(worst, check_rel(rel, want_rel, (key, c["pair"], c["delta"])))
    print(f"t2_scan {key} near level: max |rel_out - oracle| {worst:.3e}")


# ------------------------------------------------------------------ ofdm_find_preamble
def run_find_preamble(m, d_x, n, starts):
    starts = np.ascontiguousarray(starts, np.int32)
    idx = i32_out(len(starts))
    m.find_preamble(d_x, n, dev(starts), len(starts), idx)
    h = host(idx)
    assert np.all(h[len(starts):] == SENT), "written past the range"
    return h[:len(starts)].tolist()


def run_preamble_corr(m, d_x, n, start, cycles):
    out = f64_out(cycles)
    m.preamble_corr(d_x, n, start, out)
    h = host(out)
    assert np.all(h[cycles:] == 9.0), "written past the range"
    return h[:cycles]


def check_preamble_corr(m, pair, d_x, x, n, start, answer):
    """preamble_corr at one start against find_corr_ref; its first lag above
    the level is find_preamble's answer. Returns (rel_err, closed gates)."""
    C, tpl = DC.pre_cycles(pair), DC.pre_template(pair)
    level = DC.pre_config(pair)["pr_level"] / 1000
    ref, norms = DC.find_corr_ref(x, n, start, tpl, C)
    assert np.abs(norms - 1.0).min() > 1e-6, "a norm at the gate: rounding could flip it"
    got = run_preamble_corr(m, d_x, n, start, C)
    closed = norms <= 1.0
    assert np.all(got[closed] == 0.0), "a value behind a closed gate"
    err = rel_err(got, ref) if ref.any() else float(np.abs(got).max())
    assert err < 1e-10, (pair, start, err)
    above = np.nonzero(got > level)[0]
    assert answer == (start + int(above[0]) if above.size else -10), (pair, start)
    return err, int(closed.sum())


@pytest.mark.parametrize("pair", DC.PRE_PAIRS, ids=lambda p: f"L{p[0]}-T{p[1]}")
def test_find_preamble_and_preamble_corr(pair):
    m = modem(DC.pre_config(pair))
    worst = 0.0
    for texture in DC.PRE_TEXTURES:
        s = DC.pre_stream(pair, texture)
        x, n = s["x"], s["n"]
        d_x = dev(x)
        few = [st for _, st in s["starts"]]
        want_many = DC.pre_want(pair, x, n, s["many"])
        # at most 64 starts: split over workgroups; 100: one workgroup each
        got_few, got_many = run_find_preamble(m, d_x, n, few), run_find_preamble(m, d_x, n, s["many"])
        assert got_many == want_many, (pair, texture, "one workgroup per start")
        assert got_few == want_many[:len(few)], (pair, texture, "split")
        assert -10 in got_few and any(g != -10 for g in got_few)
        for tag, nc, st in s["cuts"]:  # n below the buffer
            want = DC.pre_want(pair, x, nc, [st])
            assert run_find_preamble(m, d_x, nc, [st]) == want, (pair, texture, tag, "split")
            assert run_find_preamble(m, d_x, nc, [st] * 65) == want * 65, (pair, texture, tag, "one workgroup")
        answers = dict(zip([t for t, _ in s["starts"]], got_few))
        closed = 0
        for tag in DC.PRE_CORR_TAGS:
            err, nclosed = check_preamble_corr(m, pair, d_x, x, n, dict(s["starts"])[tag], answers[tag])
            worst, closed = max(worst, err), closed + nclosed
        if texture != "f64":
            assert closed > 0, "no closed gate seen"
        assert unmodified(d_x, x), "the input was modified"
    print(f"preamble_corr {pair}: max rel_err {worst:.3e}")


@pytest.mark.parametrize("pair", DC.NEAR_PAIRS, ids=lambda p: f"L{p[0]}-T{p[1]}")
def test_find_preamble_near_the_level(pair):
    """The first passing lag's ratio at level (1 + d) and level (1 - d), d =
    1e-9, 1e-11, 1e-13: the + case stops there, the - case goes on. Both
    launch forms, and preamble_corr's first lag above the level."""
    m = modem(DC.pre_config(pair))
    cases = DC.near_level_cases(pair)
    for up, down in zip(cases[0::2], cases[1::2]):
        assert up["want"] == up["start"] + up["lag"] and down["want"] != up["want"]  # the pair reveals the decision
    for c in cases:
        d_x = dev(c["x"])
        st = c["start"]
        assert run_find_preamble(m, d_x, c["n"], [st, st - 3])[0] == c["want"], (pair, c["d"], c["sign"], "split")
        assert run_find_preamble(m, d_x, c["n"], [st] * 65) == [c["want"]] * 65, (pair, c["d"], c["sign"])
        check_preamble_corr(m, pair, d_x, c["x"], c["n"], st, c["want"])


# ------------------------------------------------------------------ ofdm_cfo_estimate
def run_cfo(m, d_x, case, nsym):
    nf = len(case["kinds"])
    out = f64_out(nf)
    m.cfo_estimate(d_x, nf, case["stride"], nsym, out)
    h = host(out)
    assert np.all(h[nf:] == 9.0), "written past the range"
    return h[:nf]


def cfo_equal(got, want):
    return np.array_equal(got.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("form", DC.CFO_FORMS, ids=lambda f: f"N{f[0]}-cp{f[1]}-x{f[2]}")
def test_cfo_estimate(form):
    """Every frame's estimate bitwise the oracle's (a mean of integer bin
    indices): 4 impaired frames, an all-zero form and a unit impulse (every
    window's maximum is its first bin)."""
    c = DC.cfo_case(form)
    m = modem(DC.cfo_config(form[0], form[1]))
    d_x = dev(c["x"])
    got = run_cfo(m, d_x, c, form[2])
    assert cfo_equal(got, c["want"]), (form, c["instance"], got, c["want"])
    assert unmodified(d_x, c["x"]), "the input was modified"


@pytest.mark.parametrize("n,cp,nsyms", [(64, 0, (1, 2)), (256, 64, (2, 1)), (512, 0, (8, 1))])
def test_cfo_estimate_keeps_a_plan_per_form_length(n, cp, nsyms):
    """A second form length on the same context builds a new plan; the first
    form is answered as before afterwards."""
    m = M.Modem(DC.cfo_config(n, cp), 0)  # a fresh context: both plans are built here
    a, b = (DC.cfo_case((n, cp, s)) for s in nsyms)
    d_a, d_b = dev(a["x"]), dev(b["x"])
    try:
        for case, d_x, nsym in ((a, d_a, nsyms[0]), (b, d_b, nsyms[1]), (a, d_a, nsyms[0]), (b, d_b, nsyms[1])):
            assert cfo_equal(run_cfo(m, d_x, case, nsym), case["want"]), (n, cp, nsym)
    finally:
        m.close()


# ------------------------------------------------------------------ status codes
def test_find_preamble_refuses_what_it_cannot_run():
    """T2sin_size = 4096 needs more LDS than a workgroup has: find_preamble
    and preamble_corr answer OFDM_ERR_UNSUPPORTED and write nothing, t2_scan on
    the same context works. nstarts = 65536: OFDM_ERR_INVALID. nstarts = 0:
    OFDM_OK and no write."""
    c = DC.t2_case("t2sin4096")
    cfg, x = c["cfg"], c["streams"]["plain"]
    m = modem(cfg)
    d_x = dev(x)
    cycles = 2 * cfg["t2sin_size"] + cfg["pr_sin_len"]
    for ns in (1, 3, 100):
        idx, d_starts = i32_out(ns), dev(np.arange(ns, dtype=np.int32) * 50)
        with pytest.raises(M.OfdmError) as e:
            m.find_preamble(d_x, len(x), d_starts, ns, idx)
        assert e.value.code == ERR_UNSUPPORTED and "T2sin_size" in str(e.value) and "pr_sin_len" in str(e.value)
        assert np.all(host(idx) == SENT)
    cor = f64_out(cycles)
    with pytest.raises(M.OfdmError) as e:
        m.preamble_corr(d_x, len(x), 100, cor)
    assert e.value.code == ERR_UNSUPPORTED and "T2sin_size" in str(e.value) and "pr_sin_len" in str(e.value)
    assert np.all(host(cor) == 9.0)
    scan = c["scans"][0]
    want_first, want_rel = DC.t2_want("t2sin4096", scan)
    first, rel = run_t2_scan(m, d_x, scan[2], scan[3], len(want_rel))
    assert first == want_first >= 0
    check_rel(rel, want_rel, "t2sin4096 after the refusals")

    s = DC.pre_stream((128, 256), "f64")
    m, d_x = modem(DC.pre_config((128, 256))), dev(s["x"])
    ns = 65536
    idx, d_starts = i32_out(ns), dev(np.zeros(ns, np.int32))
    with pytest.raises(M.OfdmError) as e:
        m.find_preamble(d_x, s["n"], d_starts, ns, idx)
    assert e.value.code == ERR_INVALID and "nstarts" in str(e.value)
    assert np.all(host(idx) == SENT)
    m.find_preamble(d_x, s["n"], d_starts, 0, idx)
    m.find_preamble(d_x, s["n"], None, 0, None)
    assert np.all(host(idx) == SENT)
    # the context still answers
    few = [st for _, st in s["starts"]]
    assert run_find_preamble(m, d_x, s["n"], few) == DC.pre_want((128, 256), s["x"], s["n"], few)
