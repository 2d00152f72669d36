"""The device transforms against a longdouble DFT, called directly through the
test-only library (c-ofdm_amd/devtest, tests/devtest.py) on chosen inputs.

FP64 forms (ofdm_fft.hpp): fft_block<LOGN, +-1> for LOGN 6..12,
fft_block_active<LOGN, -1> for LOGN 9..12, fft_regs_wave<LOGN, +-1> for LOGN
6..9. FP32 form: fft_regs_wave32p<LOGT, -1> for LOGT 6..9 (ofdm_fft32.hpp, the
stream walker's T2 screen), both packed lanes.

Inputs: impulses (every index for N <= 512; for larger N the first and last 64
indices, the powers of two and their neighbours and 64 random ones), single
tones (every bin for N <= 512, 256 bins beyond), DC and Nyquist, Gaussian
noise at 1e-3, 1 and 3e4, int16-valued blocks, a 1e4 tone over 1e-3 noise; for
the FP32 form also magnitudes near 1e-18 and 1e14.

Bars. The project's own error model: relative l2 error
<= 9 log2(N) u, u = 2^-53 or 2^-24; an index, permutation or twiddle-selection
error is O(1) on an impulse. FP64 forms also stay within RATIO x the error of
the oracle's plain C double FFT on the same input against the same reference
(impulses, on which the oracle is exact: x max(its error, 0.5 u sqrt(log2 N))).
RATIO = 8: the kernel's twiddle is a product of two table entries (<~ 3u each)
against the oracle's directly evaluated ones (<= 1u), times 2 for the
operation order. The packed FP32 form's lane B is bit-identical whatever lane A
holds, and the other way round. The worst relative error of every form and
size is printed (pytest -s)."""
import numpy as np
import pytest

import devtest as dt
import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# the reference's precision: x87 longdouble (eps 2^-63), or devtest.dft_ref's mpmath fallback (40 digits)
REF_EPS = float(np.finfo(dt.LD).eps) if dt.LD_OK else 1e-40
assert REF_EPS <= 2.0 ** -63

U64, U32 = 2.0 ** -53, 2.0 ** -24
RATIO = 8.0  # FP64 regression bar over the oracle's own error (module docstring); measured worst 3.52


def model_bar(logn, u):
    return 9.0 * logn * u


def impulse_indices(n, rng):
    if n <= 512:
        return np.arange(n)
    idx = set(range(64)) | set(range(n - 64, n))
    for m in range(0, n.bit_length() - 1):
        idx |= {(1 << m) - 1, 1 << m, (1 << m) + 1}
    idx |= set(rng.integers(0, n, 64).tolist())
    return np.array(sorted(i for i in idx if 0 <= i < n))


def tone(n, b, ampl=1.0):
    j = np.arange(n)
    return ampl * np.exp(2j * np.pi * ((b * j) % n) / n)


def cnoise(rng, rows, n, scale):
    return (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))) * scale


_sets = {}


def input_set(logn):
    """(impulse indices, other rows, their families) for N = 2^logn, built once."""
    if logn not in _sets:
        n = 1 << logn
        rng = np.random.default_rng(1000 + logn)
        imp = impulse_indices(n, rng)
        bins = np.arange(n) if n <= 512 else np.sort(rng.choice(n, 256, replace=False))
        rows, fam = [], []

        def add(name, block):
            block = np.atleast_2d(block)
            rows.append(block)
            fam.extend([name] * len(block))

        add("tone", np.stack([tone(n, b) for b in bins]))
        add("dc", np.ones(n, np.complex128))
        add("nyquist", tone(n, n // 2).real.round() + 0j)
        for s in (1e-3, 1.0, 3e4):
            add(f"noise{s:g}", cnoise(rng, 4, n, s))
        add("int16", rng.integers(-32767, 32768, (4, n)) + 1j * rng.integers(-32767, 32768, (4, n)))
        add("tone+noise", np.stack([tone(n, int(b), 1e4) for b in rng.integers(0, n, 4)]) + cnoise(rng, 4, n, 1e-3))
        _sets[logn] = (imp, np.concatenate(rows).astype(np.complex128), np.array(fam))
    return _sets[logn]


_refs = {}


def reference(logn, sign):
    """The whole input set of N = 2^logn (impulses first), its longdouble DFT,
    the oracle's relative error on every row (impulse rows floored) and the
    rows' families: computed once and shared by the forms."""
    key = (logn, sign)
    if key not in _refs:
        n = 1 << logn
        imp, other, fam = input_set(logn)
        pulses = np.zeros((len(imp), n), np.complex128)
        pulses[np.arange(len(imp)), imp] = 1.0
        x = np.concatenate([pulses, other])
        ref = np.concatenate([dt.impulse_dft(n, imp, sign), dt.dft_ref(other, sign)])
        orc = dt.rel_l2(np.stack([O.fft(r, sign) for r in x]), ref)
        orc[:len(imp)] = np.maximum(orc[:len(imp)], 0.5 * U64 * np.sqrt(logn))
        fam = np.concatenate([np.array(["impulse"] * len(imp)), fam])
        for a in (x, ref, orc, fam):
            a.setflags(write=False)
        _refs[key] = (x, ref, orc, fam)
    return _refs[key]


@pytest.mark.parametrize("form,logn,sign", dt.FFT64_FORMS,
                         ids=[f"{dt.FFT_FORM_NAMES[f]}-{1 << n}-{'fwd' if s < 0 else 'inv'}" for f, n, s in dt.FFT64_FORMS])
def test_fp64_transform_against_longdouble(form, logn, sign):
    x, ref, orc, fam = reference(logn, sign)
    err = dt.rel_l2(dt.fft64(form, logn, sign, x), ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / orc, 0.0)
    w, r = int(err.argmax()), int(ratio.argmax())
    print(f"\n{dt.FFT_FORM_NAMES[form]} N={1 << logn} sign={sign:+d}: worst rel l2 {err[w]:.3e} ({err[w] / U64:.2f} u, "
          f"{fam[w]} row {w}); model bar {model_bar(logn, U64):.3e}; worst ratio to the oracle {ratio[r]:.2f} "
          f"({fam[r]} row {r}: {err[r]:.3e} vs {orc[r]:.3e})")
    assert np.all(np.isfinite(err))
    assert err.max() <= model_bar(logn, U64), (fam[w], w, err[w])
    assert np.all(err <= RATIO * orc), (fam[r], r, err[r], orc[r])


def fp32_inputs(logt):
    """The FP64 input set plus noise at the magnitudes whose energies straddle
    the screen's 1e-20 / 1e30 guards."""
    n = 1 << logt
    x, ref, _, fam = reference(logt, -1)
    rng = np.random.default_rng(2000 + logt)
    extra = np.concatenate([cnoise(rng, 4, n, 1e-18), cnoise(rng, 4, n, 1e14)])
    return (np.concatenate([x, extra]), np.concatenate([ref, dt.dft_ref(extra, -1)]),
            np.concatenate([fam, np.array(["tiny"] * 4 + ["huge"] * 4)]))


@pytest.mark.parametrize("logt", [6, 7, 8, 9])
def test_packed_fp32_transform_against_longdouble(logt):
    x, ref, fam = fp32_inputs(logt)
    # every row through lane A (beside the reversed set) and through lane B
    XA, XB, _, _ = dt.fft32p(logt, x, x[::-1])
    for lane, got in (("A", XA), ("B", XB[::-1])):
        err = dt.rel_l2(got, ref)
        w = int(err.argmax())
        print(f"\nfft_regs_wave32p N={1 << logt} lane {lane}: worst rel l2 {err[w]:.3e} ({err[w] / U32:.2f} u, "
              f"{fam[w]} row {w}); model bar {model_bar(logt, U32):.3e}")
        assert np.all(np.isfinite(err))
        assert err.max() <= model_bar(logt, U32), (lane, fam[w], w, err[w])


@pytest.mark.parametrize("logt", [6, 7, 8, 9])
def test_packed_lanes_are_independent(logt):
    n = 1 << logt
    rng = np.random.default_rng(3000 + logt)
    keep = np.concatenate([cnoise(rng, 3, n, 1.0), cnoise(rng, 2, n, 1e-3),
                           rng.integers(-32767, 32768, (2, n)) + 1j * rng.integers(-32767, 32768, (2, n)),
                           np.stack([tone(n, 5, 1e4)]) + cnoise(rng, 1, n, 1e-3)])
    others = [np.zeros_like(keep), cnoise(rng, len(keep), n, 1e-3), np.stack([tone(n, 3 + i, 3e4) for i in range(len(keep))])]
    mask = (2, 9, 20, 27)
    outs_b = [dt.fft32p(logt, o, keep, mask, 0.8, 4e-5) for o in others]
    outs_a = [dt.fft32p(logt, keep, o, mask, 0.8, 4e-5) for o in others]
    for XA, XB, sums, verdict in outs_b[1:]:
        assert np.array_equal(XB.view(np.uint32), outs_b[0][1].view(np.uint32))
        assert np.array_equal(sums[:, 2:].view(np.uint32), outs_b[0][2][:, 2:].view(np.uint32))
        assert np.array_equal(verdict[:, 1], outs_b[0][3][:, 1])
    for XA, XB, sums, verdict in outs_a[1:]:
        assert np.array_equal(XA.view(np.uint32), outs_a[0][0].view(np.uint32))
        assert np.array_equal(sums[:, :2].view(np.uint32), outs_a[0][2][:, :2].view(np.uint32))
        assert np.array_equal(verdict[:, 0], outs_a[0][3][:, 0])
    # and a block gives the same bits in either lane
    assert np.array_equal(outs_a[0][0].view(np.uint32), outs_b[0][1].view(np.uint32))
    assert np.array_equal(outs_a[0][2][:, :2].view(np.uint32), outs_b[0][2][:, 2:].view(np.uint32))
