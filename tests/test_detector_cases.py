"""The fixtures of tests/test_gpu_detectors.py (tests/detector_cases.py),
checked on the CPU with the oracle alone: the tables reach every kernel
instance and path they are meant to, every answer a detector can give is seen
in them, no case but the crafted ones lies close enough to a threshold or a tie
for rounding to decide it, and the crafted near-level pairs sit where they say
and are decided differently by the oracle. Without that the GPU test could
pass blind.

What the GPU test is expected to notice, one wrong kernel each (scratch
builds, never committed):
- t2_scan_kernel's W0 set to 16 for every T < 64 (right for size 256 alone):
  sizes 64 and 128 fail (T = 8, 16: the xor by 16 adds a neighbouring block's
  lanes into the sums), every other size passes; the golden config, the only
  size the suite ran before, cannot see it.
- find_preamble_kernel's `j < L` tail loop dropped: the pairs with L % 8 != 0
  fail (L = 13, 100, 257: answers and preamble_corr values, near-level cases
  included), L = 8, 128 and 640 pass.
- the screen's b halved: nothing fails, and no input can make it. b is twice
  a bound that charges every prefix sum n + 512 rounded adds where the scan
  performs at most 2 ceil(n / 256) + 9 on any path (a thread's run, six wave
  steps, three wave totals, the run again), so b / 2 is still a certified
  bound and the exact recurrence decides every candidate as before. The
  near-level pairs (level (1 +- 1e-13), inside b / W of about 3e-12) stay
  candidates and are decided by the exact test either way.
- cfo_kernel's butterfly keeping the higher index on a tie: every form fails
  on its all-zero and its impulse frame (each lane's first bin ties with the
  others'; the window's first maximum is the lowest), the impaired frames
  pass."""
import numpy as np
import pytest

import detector_cases as DC
import oracle as O


# ------------------------------------------------------------------ coverage
def test_tables_cover_every_instance_and_path():
    sizes = sorted(c["t2sin_size"] for k, c in DC.T2_CONFIGS.items() if k.startswith("t2sin"))
    assert sizes == [64, 128, 256, 512, 1024, 2048, 4096]
    # blocks per workgroup as T2Geo has them: T = N / 8 threads per block, 256 threads
    assert all(DC.T2_G[s] == max(1, 256 // (s // 8)) for s in sizes)
    lo, hi, ov = DC.T2_CONFIGS["low-edge"], DC.T2_CONFIGS["high-edge"], DC.T2_CONFIGS["overlap"]
    assert lo["t2sin_size"] == hi["t2sin_size"] == ov["t2sin_size"] == 256
    assert lo["t2_sin_f1"] - lo["smooth"] < 0 and hi["t2_sin_f2"] + hi["smooth"] > 255
    assert abs(ov["t2_sin_f1"] - ov["t2_sin_f2"]) <= 2 * ov["smooth"]

    assert {DC.cfo_instance(f) for f in DC.CFO_FORMS} == DC.CFO_INSTANCES and len(DC.CFO_INSTANCES) == 12
    assert len(DC.CFO_FORMS) == 17 and sum(1 for f in DC.CFO_FORMS if f[2] > 1) == 5
    for form in DC.CFO_FORMS:
        b = DC.cfo_borders(form)
        assert 0 <= min(b) and max(b) <= (form[0] + form[1]) * form[2]

    Ls = [p[0] for p in DC.PRE_PAIRS]
    Cs = [DC.pre_cycles(p) for p in DC.PRE_PAIRS]
    assert Cs == [136, 141, 356, 640, 1281, 2688, 4736]
    assert any(L % 8 for L in Ls) and any(L % 16 and not L % 8 for L in Ls) and any(C % 32 for C in Cs)
    assert any(C % 16 for C in Cs) and any(C % 256 for C in Cs)
    slices = [DC.pre_slices(p) for p in DC.PRE_PAIRS]
    assert slices == [1, 1, 2, 3, 6, 11, 19] and max(slices) >= 16
    assert DC.pre_lds_bytes((640, 2048)) == 162640 <= 160 * 1024 < DC.pre_lds_bytes((128, 4096))
    assert all(DC.pre_lds_bytes(p, split) <= 160 * 1024 for p in DC.PRE_PAIRS for split in (True, False))
    assert set(DC.NEAR_PAIRS) <= set(DC.PRE_PAIRS)


# ------------------------------------------------------------------ T2
@pytest.mark.parametrize("key", list(DC.T2_CONFIGS))
def test_t2_cases_show_both_answers_and_are_well_conditioned(key):
    c = DC.t2_case(key)
    cfg, G, T = c["cfg"], c["G"], c["cfg"]["t2sin_size"]
    level = cfg["t2_sin_level"] / 1000
    want = {s[0]: DC.t2_want(key, s) for s in c["scans"]}
    scans = {s[0]: s for s in c["scans"]}
    # both outcomes; the no-block scans; a block count that leaves dead groups
    assert want["plain-0"][0] >= 0 and want["plain-mid"][0] >= 0 and want["plain-late"][0] == -1
    assert len({want[t][0] for t in ("plain-0", "plain-1", "plain-mid")}) == 3
    for tag in ("no-block-0", "no-block-mid", "no-block-at-n"):
        _, _, n, start = scans[tag]
        assert n - start < T and want[tag][0] == -1 and len(want[tag][1]) == 0
    assert scans["no-block-0"][2] > 0 and scans["no-block-mid"][2] - scans["no-block-mid"][3] == T - 1
    if G > 1:
        assert all(len(want[t][1]) % G for t in ("cut-0", "cut-1"))
    assert any(len(want[s[0]][1]) > G for s in c["scans"]), "more than one workgroup"
    # the zero, NaN and Inf blocks lie before the first hit and are not reported
    xs = c["streams"]["special"]
    assert np.all(xs[T:2 * T] == 0) and np.isnan(xs[2 * T:3 * T].real).sum() == 1
    assert np.isinf(xs[3 * T:4 * T].imag).sum() == 1
    first, rel = want["special-0"]
    assert first >= DC.T2_HEAD * T and np.all(rel[:DC.T2_HEAD] == 0) and np.count_nonzero(rel) >= 1
    assert np.isnan(DC.t2_ratios(cfg, xs)[1:4]).all()
    assert want["special-late"][0] == -1 and want["special-cut"][0] == -1
    assert len(want["special-cut"][1]) == DC.T2_HEAD - 1 and not want["special-cut"][1].any()
    for tag in ("special-1", "special-mid"):  # off the grid the three blocks straddle: still before the hit
        assert want[tag][0] >= 4 * T
    # conditioning: every scanned block away from the level
    closest = np.inf
    for tag, name, n, start in c["scans"]:
        r = DC.t2_ratios(cfg, c["streams"][name][start:n])
        ok = ~np.isnan(r)
        assert np.array_equal(r[ok] > level, want[tag][1][ok] > 0) and np.all(want[tag][1][~ok] == 0)
        r = r[ok]
        if r.size:
            closest = min(closest, float(np.abs(r - level).min()))
    print(f"{key}: closest block {closest:.2e} from the level")
    assert closest >= 1e-9


# ------------------------------------------------------------------ preamble
@pytest.mark.parametrize("pair", DC.PRE_PAIRS, ids=lambda p: f"L{p[0]}-T{p[1]}")
def test_preamble_cases_show_both_answers_and_are_well_conditioned(pair):
    L, C, tpl = pair[0], DC.pre_cycles(pair), DC.pre_template(pair)
    for texture in DC.PRE_TEXTURES:
        s = DC.pre_stream(pair, texture)
        cfg, x, n = s["cfg"], s["x"], s["n"]
        level = cfg["pr_level"] / 1000
        tags = dict(s["starts"])
        assert tags["negative"] < 0 and tags["past-n"] + C + L > n and np.array_equal(s["many"][:len(tags)],
                                                                                      list(tags.values()))
        assert len(s["many"]) == 100 and len(s["starts"]) <= 64
        calls = [(n, s["many"])] + [(nc, [st]) for _, nc, st in s["cuts"]]
        assert all(nc < n for _, nc, _ in s["cuts"])
        worst_r, worst_n, seen, two_sided = np.inf, np.inf, set(), False
        for nn, starts in calls:
            want = DC.pre_want(pair, x, nn, starts)
            for st, w in zip(starts, want):
                st = int(st)
                seen.add(w == -10)
                ratio, norms = DC.corr_profile(x, nn, st, tpl, C)
                upto = C if w == -10 else w - st + 1
                gate = norms[:upto] > 1.0
                if w != -10:  # the profile agrees with the oracle on the answer
                    assert gate[-1] and ratio[upto - 1] > level and not (ratio[:upto - 1][gate[:-1]] > level).any()
                    two_sided |= bool(gate[:-1].any() and not gate[:-1].all())
                if gate.any():
                    worst_r = min(worst_r, float(np.abs(ratio[:upto][gate] - level).min()) / level)
                worst_n = min(worst_n, float(np.abs(norms[:upto] - 1.0).min()))
        print(f"{pair} {texture}: closest ratio {worst_r:.2e} (relative), closest norm {worst_n:.2e} from the gate")
        assert seen == {True, False}, "a found start and a -10"
        assert worst_r >= 1e-9 and worst_n > 1e-6
        if texture == "weak":
            assert two_sided, "lags on both sides of the gate before an answer"
        if texture == "capture":
            assert np.all(x.real == np.trunc(x.real)) and np.any(x == 0)


def test_preamble_corr_starts_keep_clear_of_the_gate():
    """preamble_corr writes every lag, so at its starts every lag's norm stays
    clear of the gate, not only those up to the answer; the capture and the
    weak stream show closed gates there."""
    for pair in DC.PRE_PAIRS:
        cases = [(texture, DC.pre_stream(pair, texture)["x"], DC.pre_stream(pair, texture)["n"],
                  dict(DC.pre_stream(pair, texture)["starts"])[tag])
                 for texture in DC.PRE_TEXTURES for tag in DC.PRE_CORR_TAGS]
        if pair in DC.NEAR_PAIRS:
            cases += [("near", c["x"], c["n"], c["start"]) for c in DC.near_level_cases(pair)]
        closed = {}
        for texture, x, n, st in cases:
            _, norms = DC.find_corr_ref(x, n, st, DC.pre_template(pair), DC.pre_cycles(pair))
            assert np.abs(norms - 1.0).min() > 1e-6, (pair, texture, st)
            closed[texture] = closed.get(texture, 0) + int((norms <= 1.0).sum())
        assert closed["capture"] > 0 and closed["weak"] > 0, (pair, closed)


def test_corr_profile_agrees_with_the_serial_reference():
    for pair in ((13, 64), (257, 512)):
        s = DC.pre_stream(pair, "weak")
        for _, st in s["starts"][:4]:
            cor, norms = DC.find_corr_ref(s["x"], s["n"], st, DC.pre_template(pair), DC.pre_cycles(pair))
            ratio, pn = DC.corr_profile(s["x"], s["n"], st, DC.pre_template(pair), DC.pre_cycles(pair))
            gate = norms > 1.0
            assert np.abs(pn - norms).max() < 1e-9 and np.abs(ratio[gate] - cor[gate]).max() < 1e-9
            assert np.all(cor[~gate] == 0)


@pytest.mark.parametrize("pair", DC.NEAR_PAIRS, ids=lambda p: f"L{p[0]}-T{p[1]}")
def test_near_level_pairs_sit_where_they_say(pair):
    cases = DC.near_level_cases(pair)
    level = DC.pre_config(pair)["pr_level"] / 1000
    assert [c["d"] for c in cases[0::2]] == list(DC.NEAR_D)
    for up, down in zip(cases[0::2], cases[1::2]):
        assert up["d"] == down["d"] and up["sign"] == 1 and down["sign"] == -1
        for c in (up, down):
            assert abs(c["achieved"] / (c["sign"] * c["d"]) - 1) <= 0.1, (pair, c["d"], c["sign"], c["achieved"])
            assert (c["ratio"] > level) == (c["sign"] > 0)
        assert up["want"] == up["start"] + up["lag"]
        assert down["want"] == -10 or down["want"] > up["want"]


# ------------------------------------------------------------------ CFO
@pytest.mark.parametrize("form", DC.CFO_FORMS, ids=lambda f: f"N{f[0]}-cp{f[1]}-x{f[2]}")
def test_cfo_cases_are_distinct_and_free_of_ties(form):
    c = DC.cfo_case(form)
    S, stride = c["S"], c["stride"]
    assert stride > S and c["kinds"] == ["impaired"] * 4 + ["zeros", "impulse"]
    assert len(set(c["want"][:4].tolist())) >= 3
    gaps = np.concatenate([DC.cfo_window_gaps(form, c["x"][f * stride: f * stride + S]) for f in range(4)])
    print(f"{form}: closest two maxima of a window {gaps.min():.2e} apart (relative)")
    assert gaps.min() >= 1e-9
    # the tie frames: every window's maximum is its first bin
    b = DC.cfo_borders(form)
    p = len(b) - 2
    first = (sum(b[i] for i in range(p + 1) if i != p // 2) / p - S // 2) / S
    assert c["want"][4] == c["want"][5] == first
    assert np.all(c["x"][4 * stride: 5 * stride] == 0) and np.count_nonzero(c["x"][5 * stride:]) == 1
    assert O.pilot_freq_sinh(c["cfg"], c["x"][:S]) == c["want"][0]
