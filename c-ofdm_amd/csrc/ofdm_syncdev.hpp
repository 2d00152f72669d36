// ofdm_syncdev.hpp — device helpers of the rx sync front end shared by
// ofdm_sync.hip and ofdm_stream_wide.hip: g++-rounded complex products and
// sums, wave and workgroup sums, chan_char_lq's parallel unwrap, the stream
// sample load (f64 or complex<int16>), and every step of the sync stage that
// more than one kernel runs with the same arithmetic, operation for
// operation (the window argmax and the CFO, the radix-5 combine, the phase
// prefix, the preamble's carrier ratio, the line fit and its angle).
// Steps that two kernels round differently on purpose stay in the kernels.
// Every body carries its own `fp contract(off)`: the sync arithmetic mirrors
// the reference's x86-64 build (no FMA) wherever the header is included.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <climits>

#include "ofdm_fft.hpp"

namespace ofdm {
namespace {

__device__ __forceinline__ double2 cconj_mul(double2 a, double2 b)  // conj(a) * b, as g++ (no FMA)
{
    return cmul_exact(make_double2(a.x, -a.y), b);
}

__device__ __forceinline__ double2 cadd_rn(double2 a, double2 b)
{
    return make_double2(add_rn(a.x, b.x), add_rn(a.y, b.y));
}

// Butterfly sum over 2 * W0 aligned lanes (a wave, or a T-lane fragment of
// one with W0 = T / 2): every lane ends with the sum.
template <int W0 = 32>
__device__ __forceinline__ double2 wave_sum2(double2 v)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int o = W0; o > 0; o >>= 1) {
        v.x += __shfl_xor(v.x, o);
        v.y += __shfl_xor(v.y, o);
    }
    return v;
}

// Block-wide complex / double sums (NT threads, multiple of 64 or < 64).
template <int NT>
__device__ __forceinline__ double2 block_sum2(double2 v, double2* red)
{
#pragma clang fp contract(off)
    // wave_sum2's loop, written out: through the call the N = 4096 wide decode
    // kernel comes out two instructions shorter, and its code is pinned
    constexpr int W0 = NT >= 64 ? 32 : NT / 2;
#pragma unroll
    for (int o = W0; o > 0; o >>= 1) {
        v.x += __shfl_xor(v.x, o);
        v.y += __shfl_xor(v.y, o);
    }
    constexpr int NW = (NT + 63) / 64;
    if constexpr (NW == 1) {
        return v;
    } else {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        __syncthreads();
        if (lane == 0) red[w] = v;
        __syncthreads();
        double2 s = make_double2(0.0, 0.0);
#pragma unroll
        for (int i = 0; i < NW; ++i) s = cadd(s, red[i]);
        return s;
    }
}

// ---------------------------------------------------------------- unwrap
// chan_char_lq's one-pass unwrap (Frame.hpp:407-414: a phase moves by -/+2 pi
// when it differs from the already-adjusted previous one by more than pi) as
// a parallel scan. Entry i's rule maps the previous entry's adjustment
// k in {-1, 0, +1} (state k+1) to its own, so each entry is a map on 3
// states, 2 bits per state; maps compose associatively. Per state the same
// FP64 operations as the serial loop run, so the result is bit-identical.
constexpr unsigned UMAP_ID = 0u | (1u << 2) | (2u << 4);

__device__ __forceinline__ unsigned umap_then(unsigned f, unsigned g)  // f, then g
{
    unsigned h = 0;
#pragma unroll
    for (int s = 0; s < 3; ++s) h |= ((g >> (2 * ((f >> (2 * s)) & 3))) & 3) << (2 * s);
    return h;
}

// ph[0..n) raw phases in LDS (visible to every thread); on return they are
// unwrapped and visible. All NT threads call it; scr: NT/64 words of LDS.
// n - 1 <= 4 * NT (chan_char_lq: n = D/2 <= N/2 = 4 * NT).
template <int NT, bool WAVE = false>
__device__ void unwrap_scan(double* ph, int n, unsigned* scr)
{
#pragma clang fp contract(off)
    static_assert(!WAVE || NT == 64, "a wave-local scan is one wave");
    const int t = threadIdx.x, lane = t & 63;
    const int R = (n - 1 + NT - 1) / NT;  // entries 1..n-1, R consecutive per thread
    const int i0 = 1 + t * R;
    unsigned m[4];
    double raw[4];
    unsigned loc = UMAP_ID;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + r;
        m[r] = UMAP_ID;
        raw[r] = 0.0;
        if (r < R && i < n) {
            const double x = ph[i], prev = ph[i - 1];
            raw[r] = x;
            unsigned mr = 0;
#pragma unroll
            for (int st = 0; st < 3; ++st) {
                const double pa = st == 1 ? prev : (st == 0 ? prev - 2 * M_PI : prev + 2 * M_PI);
                const double d = x - pa;
                mr |= (d > M_PI ? 0u : (d < -M_PI ? 2u : 1u)) << (2 * st);
            }
            m[r] = mr;
            loc = umap_then(loc, mr);
        }
    }
    // exclusive scan of the per-thread maps (wave shuffles, then wave totals)
    unsigned inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(inc, o);
        if (lane >= o) inc = umap_then(y, inc);
    }
    unsigned ex = __shfl_up(inc, 1);
    if (lane == 0) ex = UMAP_ID;
    if constexpr (NT > 64) {
        if (lane == 63) scr[t >> 6] = inc;
        __syncthreads();
        unsigned pre = UMAP_ID;
        for (int w = 0; w < (t >> 6); ++w) pre = umap_then(pre, scr[w]);
        ex = umap_then(pre, ex);
    }
    if constexpr (WAVE)
        wave_lds_sync();
    else
        __syncthreads();  // every raw phase has been read
    int st = (ex >> 2) & 3;  // entry 0 is never adjusted (state 1)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + r;
        if (r < R && i < n) {
            st = (m[r] >> (2 * st)) & 3;
            ph[i] = st == 1 ? raw[r] : (st == 0 ? raw[r] - 2 * M_PI : raw[r] + 2 * M_PI);
        }
    }
    if constexpr (WAVE)
        wave_lds_sync();
    else
        __syncthreads();
}

// One stream sample as complex<double> (f64 stream, or complex<int16>
// converted exactly: FRAME_FORM::form_int16_to_double, Frame.hpp:472-481).
__device__ __forceinline__ double2 src_sample(const double2* iq, const short2* iq16, long j)
{
    if (iq16) {
        const short2 w = iq16[j];
        return make_double2((double)w.x, (double)w.y);
    }
    return iq[j];
}

// src_sample with the stream's format fixed at compile time (kernels
// instantiated per format): no per-sample branch between the loads, so an
// unrolled loop issues its loads back to back.
template <bool I16>
__device__ __forceinline__ double2 src_sample_t(const double2* iq, const short2* iq16, long j)
{
    if constexpr (I16) {
        const short2 w = iq16[j];
        return make_double2((double)w.x, (double)w.y);
    } else {
        return iq[j];
    }
}

// ---------------------------------------------------------------- pilot_freq_sinh
// First maximum of mag(j) over window [lo, hi) (std::max_element:
// strictly-greater keeps the first maximum) by a group of ARGMAX_LANES lanes,
// aligned within a wave: lane l takes the first maximum of its strided share,
// then a butterfly keeps the larger value, the lower index on ties. Every
// lane of the group returns the index (INT_MAX for an empty window). The
// caller applies max_element's other two rules: an empty range gives hi, and
// a NaN first element is kept (nothing compares greater than it).
constexpr int ARGMAX_LANES = 8;

template <class Mag>
__device__ __forceinline__ int window_first_max(int lo, int hi, int l, Mag mag)
{
#pragma clang fp contract(off)
    double bv = -1.0;  // below every magnitude
    int bi = INT_MAX;
    for (int j = lo + l; j < hi; j += ARGMAX_LANES) {
        const double h = mag(j);
        if (bv < h) {
            bv = h;
            bi = j;
        }
    }
#pragma unroll
    for (int o = 1; o < ARGMAX_LANES; o <<= 1) {
        const double ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
        }
    }
    return bi;
}

// wsum[i] = first argmax of |X| = hypot over spec's pilot window [borders[i],
// borders[i+1]) for the P windows i != P/2 (the CFO sum skips that one), by
// the NT threads of the workgroup (tid, in wave w). Decided on e = |X|^2 (two
// products, one sum: relative error <= 2u, u = 2^-53) where the runner-up e2
// < e1 * (1 - 64u): then every other element's hypot (error <= 4u) is
// strictly below the winner's, so the winner is hypot's first maximum.
// Otherwise (near-ties, or a non-finite element) the group takes hypot of its
// window, as cfo_kernel does. A wave whose groups are all past the last
// window skips the pass (a uniform branch): for P <= 8 wave 0 works alone.
template <int NT>
__device__ __forceinline__ void window_argmax_screened(const double2* spec, const int* borders, int P, int* wsum,
                                                       int tid, int w)
{
#pragma clang fp contract(off)
    constexpr int AG = ARGMAX_LANES;
    constexpr double SURE = 1.0 - 64.0 * 0x1.0p-53;
    for (int g0 = 0; g0 < P; g0 += NT / AG) {
        if (g0 + w * (64 / AG) >= P) continue;  // uniform per wave
        const int gi = g0 + tid / AG, l = tid % AG;
        const int i = gi < P / 2 ? gi : gi + 1;
        const bool act = gi < P;
        int lo = 0, hi = 0;
        if (act) {
            lo = borders[i];
            hi = borders[i + 1];
        }
        double bv = -1.0, sv = -1.0;  // best and runner-up |X|^2 (below every magnitude)
        int bi = INT_MAX, odd = 0;
        for (int j = lo + l; j < hi; j += AG) {
            const double2 z = spec[j];
            const double e = add_rn(mul_rn(z.x, z.x), mul_rn(z.y, z.y));
            odd |= !(e <= DBL_MAX);  // NaN or inf: hypot decides
            if (bv < e) {
                sv = bv;
                bv = e;
                bi = j;
            } else if (sv < e) {
                sv = e;
            }
        }
#pragma unroll
        for (int o = 1; o < AG; o <<= 1) {
            const double ov = __shfl_xor(bv, o), os = __shfl_xor(sv, o);
            const int oi = __shfl_xor(bi, o);
            odd |= __shfl_xor(odd, o);
            if (ov > bv || (ov == bv && oi < bi)) {
                sv = fmax(bv, fmax(sv, os));
                bv = ov;
                bi = oi;
            } else {
                sv = fmax(sv, fmax(ov, os));
            }
        }
        bool first_nan = false;
        if (odd || !(sv < bv * SURE)) {  // uniform within the 8-lane group
            bi = window_first_max(lo, hi, l, [&](int j) { return hypot(spec[j].x, spec[j].y); });
            first_nan = lo < hi && isnan(hypot(spec[lo].x, spec[lo].y));
        }
        if (act && l == 0) wsum[i] = lo < hi ? (first_nan ? lo : bi) : hi;
    }
}

// The shift from the window maxima: their mean over the P windows i != P/2,
// recentred on the fftshifted spectrum's middle, in cycles per sample
// (Frame.hpp:324-336). One thread.
__device__ __forceinline__ double cfo_from_windows(const int* wsum, int P, int S)
{
#pragma clang fp contract(off)
    double shift = 0.0;
    for (int i = 0; i <= P; ++i)
        if (i != P / 2) shift += wsum[i];
    shift /= P;
    shift -= S / 2;
    shift /= S;
    return shift;
}

// The 5-point DFT over q by the symmetric pairs (1, 4), (2, 3): X_r, X_{5-r}
// = t_r +- i u_r, with W5 = w1 = (c1, n1), W5^2 = w2 = (c2, n2) (44
// operations instead of 20 products + sums).
__device__ __forceinline__ void radix5_combine(const double2 (&tq)[5], double2 w1, double2 w2, double2 (&X)[5])
{
#pragma clang fp contract(off)
    const double c1 = w1.x, n1 = w1.y, c2 = w2.x, n2 = w2.y;
    const double2 a0 = tq[0];
    const double2 s1 = make_double2(tq[1].x + tq[4].x, tq[1].y + tq[4].y);
    const double2 d1 = make_double2(tq[1].x - tq[4].x, tq[1].y - tq[4].y);
    const double2 s2 = make_double2(tq[2].x + tq[3].x, tq[2].y + tq[3].y);
    const double2 d2 = make_double2(tq[2].x - tq[3].x, tq[2].y - tq[3].y);
    const double2 t1 = make_double2(a0.x + c1 * s1.x + c2 * s2.x, a0.y + c1 * s1.y + c2 * s2.y);
    const double2 t2 = make_double2(a0.x + c2 * s1.x + c1 * s2.x, a0.y + c2 * s1.y + c1 * s2.y);
    const double2 u1 = make_double2(n1 * d1.x + n2 * d2.x, n1 * d1.y + n2 * d2.y);
    const double2 u2 = make_double2(n2 * d1.x - n1 * d2.x, n2 * d1.y - n1 * d2.y);
    X[0] = make_double2(a0.x + s1.x + s2.x, a0.y + s1.y + s2.y);
    X[1] = make_double2(t1.x - u1.y, t1.y + u1.x);
    X[2] = make_double2(t2.x - u2.y, t2.y + u2.x);
    X[3] = make_double2(t2.x + u2.y, t2.y - u2.x);
    X[4] = make_double2(t1.x + u1.y, t1.y - u1.x);
}

// ---------------------------------------------------------------- cp_freq_sinh
// psi_q = phi_0 + ... + phi_{q-1}, in that order (Frame.hpp:257-260). One thread.
__device__ __forceinline__ void phase_prefix(const double* phi, double* psi, int n)
{
#pragma clang fp contract(off)
    double p = 0.0;
    for (int q = 0; q < n; ++q) {
        psi[q] = p;
        p += phi[q];
    }
}

// ---------------------------------------------------------------- pr_phase_sinh
// e^{-i phr}, phr = arg(acc), as conj(acc) / |acc| (acc is uniform: a uniform
// branch keeps sincos for a zero or non-finite sum).
__device__ __forceinline__ double2 unit_conj(double2 acc, double phr)
{
#pragma clang fp contract(off)
    const double ha = hypot(acc.x, acc.y);
    if (ha > 0.0 && ha <= DBL_MAX) {
        const double ir = 1.0 / ha;
        return make_double2(acc.x * ir, -acc.y * ir);
    }
    double rs, rc;
    sincos(-phr, &rs, &rc);
    return make_double2(rc, rs);
}

// ---------------------------------------------------------------- chan_char_lq
// (F/phys)/coef/mod_pre of one preamble data carrier, coef = (F[0,p]/phys) /
// (F[0,p]/phys) at the carrier's pilot slot: the reference's divisions
// verbatim (Frame.hpp:397-405 over FFT_FORM::read, Frame.cpp:82-93). d: the
// carrier's raw bin, pj: its pilot's, mp: its BPSK preamble point.
__device__ __forceinline__ double2 preamble_ratio(const double2& pj, const double2& d, const double2& mp, double phys)
{
#pragma clang fp contract(off)
    const double2 p0 = make_double2(pj.x / phys, pj.y / phys);
    const double2 coef = cdiv_exact(p0, p0);
    const double2 fs = make_double2(d.x / phys, d.y / phys);
    return cdiv_exact(cdiv_exact(fs, coef), mp);
}

// Least-squares line ph[i] ~ aa + b i over the n unwrapped phases, on raw
// sums (Frame.hpp:416-423): returns (b, aa) on every one of the NT threads t.
// red: block_sum2's slot.
template <int NT>
__device__ __forceinline__ double2 phase_line_fit(const double* ph, int n, int t, double2* red)
{
#pragma clang fp contract(off)
    double sxy = 0.0, sy = 0.0;
    for (int i = t; i < n; i += NT) {
        sxy += ph[i] * i;
        sy += ph[i];
    }
    const double2 sums = block_sum2<NT>(make_double2(sxy, sy), red);
    // integer sums are exact in any order
    const double hn = (double)n;
    const double sx = hn * (hn - 1) / 2, sx2 = (hn - 1) * hn * (2 * hn - 1) / 6;
    const double b = (sums.x - sx * sums.y) / (sx2 - sx * sx);
    return make_double2(b, sums.y - b * sx);
}

// The fitted line's angle at data carrier i of D: the first half as fitted,
// the second half continued from -b D / 2 (Frame.hpp:425-430).
__device__ __forceinline__ double chan_line_angle(double b, double aa, int half, int D, int i)
{
#pragma clang fp contract(off)
    if (i < half) return add_rn(mul_rn(b, (double)i), aa);
    return add_rn(add_rn(mul_rn(-b, (double)D) / 2, mul_rn((double)(i - half), b)), aa);
}

}  // namespace
}  // namespace ofdm
