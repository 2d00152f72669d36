// ofdm_devtest.hip — test-only launchers for device primitives that no C-ABI
// entry reaches with chosen arguments: atan2_fast / cp_phase (ofdm_fft.hpp),
// unwrap_scan and the pilot windows' plain and screened first maximum
// (ofdm_syncdev.hpp), and the rx emit's fast path (ofdm_dev.hpp):
// the threshold scan, the decision by thresholds beside decide_select, and
// the in-wave assembly of output words; and the transforms themselves
// (ofdm_fft.hpp's fft_block, fft_block_active and fft_regs_wave, ofdm_fft32.hpp's
// packed FP32 forms with the stream walker's T2 sums and screen rule and the
// FFT preamble search's window pass), on chosen inputs, with the twiddle table
// of the product's own host function.
// Built into lib/libofdm_devtest.so, a library of its own: nothing here is
// linked into libofdm_mi355x.so. Every launcher takes device pointers and a
// stream, launches one kernel and returns the launch's hipError_t.
#include <hip/hip_runtime.h>

#include <vector>

#include "../csrc/ofdm_dev.hpp"
#include "../csrc/ofdm_fft32.hpp"
#include "../csrc/ofdm_internal.hpp"
#include "../csrc/ofdm_syncdev.hpp"

namespace {

__global__ void atan2_kernel(const double* __restrict__ y, const double* __restrict__ x, double* __restrict__ out,
                             long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = ofdm::atan2_fast(y[i], x[i]);
}

// acc, rot: n complex pairs (re, im interleaved)
__global__ void cp_phase_kernel(const double2* __restrict__ acc, const double2* __restrict__ rot,
                                double* __restrict__ out, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = ofdm::cp_phase(acc[i], rot[i]);
}

// One sequence per workgroup: row b of ph (stride doubles apart, len[b]
// entries, 1 <= len[b] <= 4 * NT + 1) goes to LDS, is unwrapped there as the
// decode kernels do it, and comes back in place. The wave-local form runs in
// wave 0 of a two-wave workgroup, as in the fused stream decode.
template <int NT, bool WAVE>
__global__ void __launch_bounds__(WAVE ? 2 * NT : NT)
unwrap_kernel(double* __restrict__ ph, const int* __restrict__ len, long stride)
{
    __shared__ double lds[4 * NT + 1];
    __shared__ unsigned scr[(NT + 63) / 64];
    double* row = ph + (long)blockIdx.x * stride;
    const int n = min(len[blockIdx.x], 4 * NT + 1);
    for (int i = threadIdx.x; i < n; i += blockDim.x) lds[i] = row[i];
    __syncthreads();
    if (!WAVE || threadIdx.x < NT) ofdm::unwrap_scan<NT, WAVE>(lds, n, scr);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) row[i] = lds[i];
}

template <int NT, bool WAVE>
int launch_unwrap(double* ph, const int* len, int nseq, long stride, hipStream_t s)
{
    hipLaunchKernelGGL((unwrap_kernel<NT, WAVE>), dim3(nseq), dim3(WAVE ? 2 * NT : NT), 0, s, ph, len, stride);
    return (int)hipGetLastError();
}

// One fftshifted spectrum of S bins per workgroup, in LDS as in the decode
// kernels, with its own borders[P + 2]: the pilot windows' first maxima of
// |X| by window_first_max over hypot as cfo_kernel runs it (every window
// 0..P) into plain, and by window_argmax_screened (the windows != P/2) into
// screened; P + 1 entries each per spectrum, -1 where nothing was written.
template <int NT>
__global__ void __launch_bounds__(NT)
window_argmax_kernel(const double2* __restrict__ spec_g, const int* __restrict__ borders_g, int P, int S,
                     int* __restrict__ plain, int* __restrict__ screened)
{
    extern __shared__ double2 wa_lds[];
    double2* spec = wa_lds;
    int* wp = reinterpret_cast<int*>(spec + S);
    int* ws = wp + P + 1;
    const int tid = threadIdx.x, w = tid >> 6;
    const long b = blockIdx.x;
    const int* borders = borders_g + b * (P + 2);
    for (int i = tid; i < S; i += NT) spec[i] = spec_g[b * S + i];
    for (int i = tid; i <= P; i += NT) wp[i] = ws[i] = -1;
    __syncthreads();
    constexpr int AG = ofdm::ARGMAX_LANES;
    for (int i0 = 0; i0 <= P; i0 += NT / AG) {
        const int i = i0 + tid / AG, l = tid % AG;
        const bool act = i <= P;
        int lo = 0, hi = 0;
        if (act) {
            lo = borders[i];
            hi = borders[i + 1];
        }
        const int bi = ofdm::window_first_max(lo, hi, l, [&](int j) { return hypot(spec[j].x, spec[j].y); });
        if (act && l == 0) wp[i] = lo < hi ? (isnan(hypot(spec[lo].x, spec[lo].y)) ? lo : bi) : hi;
    }
    ofdm::window_argmax_screened<NT>(spec, borders, P, ws, tid, w);
    __syncthreads();
    for (int i = tid; i <= P; i += NT) {
        plain[b * (P + 1) + i] = wp[i];
        screened[b * (P + 1) + i] = ws[i];
    }
}

__global__ void __launch_bounds__(256) tau_scan_kernel(int k, double* out)
{
    __shared__ double lds[ofdm::DEC_TAU_MAX + 1];
    ofdm::decide_tau_scan(k, out, lds);
}

// z: n points; sel[i] = decide_select, thr[i] = decide_tau<K> with tau[0..2]
template <int K>
__global__ void decide_kernel(const double2* __restrict__ z, const double* __restrict__ tau,
                              uint8_t* __restrict__ sel, uint8_t* __restrict__ thr, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int m = 1 << (K / 2);
    const double s1 = 1.0 / (2.0 / (m - 1));  // rx_kernel's expression
    const double t[ofdm::DEC_TAU_MAX] = {tau[0], tau[1], tau[2]};
    sel[i] = (uint8_t)ofdm::decide_select(z[i], K, s1, m);
    thr[i] = (uint8_t)ofdm::decide_tau<K>(z[i], t);
}

// One wave per workgroup: bits[64 b + lane] in, emit_words' K/2 words of every
// lane out (words[(64 b + lane) * 2 + h]; h = 1 unused for K = 2).
template <int K>
__global__ void __launch_bounds__(64) emit_words_kernel(const unsigned* __restrict__ bits,
                                                        unsigned* __restrict__ words)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    unsigned w[K / 2];
    ofdm::emit_words<K>(bits[i], (int)threadIdx.x, w);
    for (int h = 0; h < K / 2; ++h) words[2 * i + h] = w[h];
}

// ---------------------------------------------------------------- transforms
// Many transforms per launch, each by the thread group the product kernels
// give it, calling the header functions as they do. x, X: transform b at
// b * N (complex, natural order). tw: ofdm::twiddles(N) on the device.

// fft_block<LOGN, SIGN> by one workgroup of N/8 threads (ACTIVE: by the first
// N/8 threads of a workgroup of twice as many, fft_block_active, the other
// half taking the barriers only).
template <int LOGN, int SIGN, bool ACTIVE>
__global__ void __launch_bounds__((ACTIVE ? 2 : 1) * (1 << LOGN) / 8)
fft_block_kernel(const double2* __restrict__ x, double2* __restrict__ X, const double2* __restrict__ tw)
{
    constexpr int N = 1 << LOGN, T = N / 8;
    extern __shared__ double2 sm[];
    double2* lds = sm;
    double2* lds_tw = sm + N;
    const int t = threadIdx.x;
    const bool active = t < T;
    ofdm::load_twiddles<LOGN>(tw, lds_tw, t, (int)blockDim.x);
    const long base = (long)blockIdx.x * N;
    double2 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = active ? x[base + t + T * i] : make_double2(0.0, 0.0);
    __syncthreads();
    if constexpr (ACTIVE)
        ofdm::fft_block_active<LOGN, SIGN>(v, t, lds_tw, lds, active);
    else
        ofdm::fft_block<LOGN, SIGN>(v, t, lds_tw, lds);
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) X[base + t + T * i] = lds[ofdm::lds_swz(t + T * i)];
    }
}

// fft_regs_wave<LOGN, SIGN>: one wave, 512/N transforms side by side (group g
// of N/8 lanes, its own image), nt transforms in all.
template <int LOGN, int SIGN>
__global__ void __launch_bounds__(64)
fft_wave_kernel(const double2* __restrict__ x, double2* __restrict__ X, const double2* __restrict__ tw, long nt)
{
    constexpr int N = 1 << LOGN, T = N / 8, G = 64 / T;
    __shared__ double2 lds[G * N];
    __shared__ double2 lds_tw[ofdm::TwLds<LOGN>::SIZE];
    const int t = threadIdx.x, g = t / T, tt = t - g * T;
    ofdm::load_twiddles<LOGN>(tw, lds_tw, t, 64);
    const long b = (long)blockIdx.x * G + g;
    const bool live = b < nt;
    const long base = (live ? b : 0) * N;
    double2 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = x[base + tt + T * i];
    __syncthreads();
    ofdm::fft_regs_wave<LOGN, SIGN>(v, tt, lds_tw, lds + g * N);
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) X[base + tt + T * i] = v[i];
    }
}

// fft_regs_wave32p<LOGT, -1> on pairs of blocks (A, B) as the stream walker's
// FP32 T2 screen runs it (ofdm_sync.hip stream_walk_kernel, the t2_f32
// branch): groups of T = N/8 lanes side by side in a wave, the f64 samples
// rounded to float as load8_block32 rounds them, one float4 image per group.
// XA, XB: the two spectra (float2); sums: {ta, sa, tb, sb} per pair; verdict:
// the screen rule's {A, B} per pair.
template <int LOGT>
__global__ void __launch_bounds__(64)
fft32p_kernel(const double2* __restrict__ xa, const double2* __restrict__ xb, float2* __restrict__ XA,
              float2* __restrict__ XB, float* __restrict__ sums, int* __restrict__ verdict,
              const double2* __restrict__ tw, long np, int a1, int b1, int a2, int b2, double t2_level,
              double t2_margin)
{
    using ofdm::PCx;
    using ofdm::pf2;
    constexpr int N = 1 << LOGT, T = N / 8, G = 64 / T;
    __shared__ float4 fftb32[G * N];
    __shared__ double2 lds_tw[ofdm::TwLds<LOGT>::SIZE];
    const int t0 = threadIdx.x, g = t0 / T, tt = t0 - g * T;
    ofdm::load_twiddles<LOGT>(tw, lds_tw, t0, 64);
    const long p = (long)blockIdx.x * G + g;
    const bool in = p < np;
    const long base = (in ? p : 0) * N;
    PCx v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double2 da = xa[base + tt + T * i], db = xb[base + tt + T * i];
        v[i] = PCx{pf2{(float)da.x, (float)db.x}, pf2{(float)da.y, (float)db.y}};
    }
    __syncthreads();
    // ---- replica of ofdm_sync.hip stream_walk_kernel, the t2_f32 branch
    // (the mask bits, the transform, the sums and the screen rule): a copy,
    // tied to the kernel by tests/test_gpu_t2_near_level.py
    const float lev = (float)t2_level, marg = (float)t2_margin;
    int mbits = 0;
    {
        const int tm = t0 & (T - 1);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = tm + T * i;
            mbits |= ((k >= a1 && k <= b1) + (k >= a2 && k <= b2)) << (2 * i);
        }
    }
    ofdm::fft_regs_wave32p<LOGT, -1>(v, tt, lds_tw, fftb32 + g * N);
    pf2 tot2 = {0.f, 0.f}, sin2 = {0.f, 0.f};
    int mb;
    asm volatile("v_mov_b32 %0, %1" : "=v"(mb) : "v"(mbits));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float m = (float)((mb >> (2 * i)) & 3);
        const pf2 e = v[i].re * v[i].re + v[i].im * v[i].im;
        tot2 += e;
        sin2 += pf2{m, m} * e;
    }
    const float ta = ofdm::group_sum<T>(tot2.x), sa = ofdm::group_sum<T>(sin2.x);
    const float tb = ofdm::group_sum<T>(tot2.y), sb = ofdm::group_sum<T>(sin2.y);
    // 0 = certain FAIL, 1 = certain PASS, 2 = uncertain
    auto screen = [&](bool live, float tot, float sine) -> int {
        if (!live) return 0;
        if (!(tot >= 1e-20f && tot <= 1e30f)) return 2;  // zero, tiny, huge or NaN: FP64 decides
        const float rel = sine / tot;
        if (rel > lev + marg) return 1;
        if (rel <= lev - marg) return 0;
        return 2;
    };
    // ---- end of the replica
    if (!in) return;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        XA[base + tt + T * i] = make_float2(v[i].re.x, v[i].im.x);
        XB[base + tt + T * i] = make_float2(v[i].re.y, v[i].im.y);
    }
    if (tt == 0) {
        sums[4 * p + 0] = ta;
        sums[4 * p + 1] = sa;
        sums[4 * p + 2] = tb;
        sums[4 * p + 3] = sb;
        verdict[2 * p + 0] = screen(true, ta, sa);
        verdict[2 * p + 1] = screen(true, tb, sb);
    }
}

// The window pass of walk_preamble_fft (ofdm_sync.hip), one wave per window
// of M = 512 samples: forward transform, product with the spectrum H, inverse
// transform, in packed FP32 (F32: the samples and H rounded to float as the
// walker and the context round them) or in FP64. c = M times the correlation.
template <bool F32>
__global__ void __launch_bounds__(64)
corr_kernel(const double2* __restrict__ x, const double2* __restrict__ H, double2* __restrict__ c_out,
            const double2* __restrict__ tw)
{
    using ofdm::pf2;
    constexpr int LM = 9, M = 1 << LM;
    __shared__ double2 buf[M];
    __shared__ double2 tw_m[ofdm::TwLds<LM>::SIZE];
    const int lane = threadIdx.x;
    ofdm::load_twiddles<LM>(tw, tw_m, lane, 64);
    const long base = (long)blockIdx.x * M;
    double2 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = x[base + lane + 64 * i];
    __syncthreads();
    const double2* tp = H + lane;
    if constexpr (F32) {
        float2 ts[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ts[i] = make_float2((float)tp[64 * i].x, (float)tp[64 * i].y);
        pf2 c[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = pf2{(float)v[i].x, (float)v[i].y};
        ofdm::fft_regs_wave32c<LM, -1>(c, lane, tw_m, buf);
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = ofdm::c_mulw(c[i], pf2{ts[i].x, ts[i].y});
        ofdm::fft_regs_wave32c<LM, +1>(c, lane, tw_m, buf);
#pragma unroll
        for (int j = 0; j < 8; ++j) c_out[base + lane + 64 * j] = make_double2((double)c[j].x, (double)c[j].y);
    } else {
        ofdm::fft_regs_wave<LM, -1>(v, lane, tw_m, buf);
        double2 ts[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ts[i] = tp[64 * i];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ofdm::cmul(v[i], ts[i]);
        ofdm::fft_regs_wave<LM, +1>(v, lane, tw_m, buf);
#pragma unroll
        for (int j = 0; j < 8; ++j) c_out[base + lane + 64 * j] = v[j];
    }
}

// ofdm::twiddles(1 << logn) on the device: built once per size with the
// product's own host function and kept for the life of the library.
const double2* device_twiddles(int logn)
{
    static double2* tab[13] = {};
    if (logn < 6 || logn > 12) return nullptr;
    if (!tab[logn]) {
        const std::vector<double2> w = ofdm::twiddles(1 << logn);
        double2* d = nullptr;
        if (hipMalloc(&d, w.size() * sizeof(double2)) != hipSuccess) return nullptr;
        if (hipMemcpy(d, w.data(), w.size() * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d);
            return nullptr;
        }
        tab[logn] = d;
    }
    return tab[logn];
}

template <int LOGN, int SIGN, bool ACTIVE>
int launch_fft_block(const double2* x, double2* X, const double2* tw, long nt, hipStream_t s)
{
    constexpr int N = 1 << LOGN;
    constexpr size_t shm = (N + ofdm::TwLds<LOGN>::SIZE) * sizeof(double2);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&fft_block_kernel<LOGN, SIGN, ACTIVE>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((fft_block_kernel<LOGN, SIGN, ACTIVE>), dim3((unsigned)nt), dim3((ACTIVE ? 2 : 1) * N / 8), shm,
                       s, x, X, tw);
    return (int)hipGetLastError();
}

template <int LOGN, int SIGN>
int launch_fft_wave(const double2* x, double2* X, const double2* tw, long nt, hipStream_t s)
{
    constexpr int G = 64 / ((1 << LOGN) / 8);
    hipLaunchKernelGGL((fft_wave_kernel<LOGN, SIGN>), dim3((unsigned)((nt + G - 1) / G)), dim3(64), 0, s, x, X, tw, nt);
    return (int)hipGetLastError();
}

template <int LOGN, int SIGN>
int launch_fft64(int form, const double2* x, double2* X, const double2* tw, long nt, hipStream_t s)
{
    if (form == 0) return launch_fft_block<LOGN, SIGN, false>(x, X, tw, nt, s);
    if constexpr (LOGN >= 9 && SIGN < 0)
        if (form == 1) return launch_fft_block<LOGN, SIGN, true>(x, X, tw, nt, s);
    if constexpr (LOGN <= 9)
        if (form == 2) return launch_fft_wave<LOGN, SIGN>(x, X, tw, nt, s);
    return -1;
}

template <int LOGN>
int launch_fft64_sign(int form, int sign, const double2* x, double2* X, const double2* tw, long nt, hipStream_t s)
{
    return sign < 0 ? launch_fft64<LOGN, -1>(form, x, X, tw, nt, s) : launch_fft64<LOGN, +1>(form, x, X, tw, nt, s);
}

}  // namespace

extern "C" {

// nt transforms of N = 2^logn points, sign -1 or +1 (unnormalised), by
// form 0: fft_block (logn 6..12), 1: fft_block_active (logn 9..12, sign -1),
// 2: fft_regs_wave (logn 6..9). -1 for a form that is not instantiated.
int ofdm_devtest_fft64(int form, int logn, int sign, const double* x, double* X, long nt, hipStream_t s)
{
    if (sign != 1 && sign != -1) return -1;
    if (nt <= 0) return 0;
    const double2* tw = device_twiddles(logn);
    if (!tw) return -1;
    const double2* xx = reinterpret_cast<const double2*>(x);
    double2* XX = reinterpret_cast<double2*>(X);
    switch (logn) {
    case 6: return launch_fft64_sign<6>(form, sign, xx, XX, tw, nt, s);
    case 7: return launch_fft64_sign<7>(form, sign, xx, XX, tw, nt, s);
    case 8: return launch_fft64_sign<8>(form, sign, xx, XX, tw, nt, s);
    case 9: return launch_fft64_sign<9>(form, sign, xx, XX, tw, nt, s);
    case 10: return launch_fft64_sign<10>(form, sign, xx, XX, tw, nt, s);
    case 11: return launch_fft64_sign<11>(form, sign, xx, XX, tw, nt, s);
    case 12: return launch_fft64_sign<12>(form, sign, xx, XX, tw, nt, s);
    default: return -1;
    }
}

// np pairs of blocks of N = 2^logt points (logt 6..9) through the walker's
// packed FP32 transform, sums and screen rule (fft32p_kernel); the detector
// mask is the two bin ranges [a1, b1] and [a2, b2], added where they overlap.
int ofdm_devtest_fft32p(int logt, const double* xa, const double* xb, float* XA, float* XB, float* sums,
                        int* verdict, long np, int a1, int b1, int a2, int b2, double level, double margin,
                        hipStream_t s)
{
    if (np <= 0) return 0;
    const double2* tw = device_twiddles(logt);
    if (!tw || logt > 9) return -1;
    const double2* pa = reinterpret_cast<const double2*>(xa);
    const double2* pb = reinterpret_cast<const double2*>(xb);
    float2* oa = reinterpret_cast<float2*>(XA);
    float2* ob = reinterpret_cast<float2*>(XB);
    const int G = 64 / ((1 << logt) / 8);
    const dim3 grid((unsigned)((np + G - 1) / G));
#define OFDM_DEVTEST_FFT32P(L)                                                                                  \
    hipLaunchKernelGGL(fft32p_kernel<L>, grid, dim3(64), 0, s, pa, pb, oa, ob, sums, verdict, tw, np, a1, b1, a2, \
                       b2, level, margin)
    switch (logt) {
    case 6: OFDM_DEVTEST_FFT32P(6); break;
    case 7: OFDM_DEVTEST_FFT32P(7); break;
    case 8: OFDM_DEVTEST_FFT32P(8); break;
    default: OFDM_DEVTEST_FFT32P(9); break;
    }
#undef OFDM_DEVTEST_FFT32P
    return (int)hipGetLastError();
}

// nw windows of 512 samples (zero tails written by the caller) correlated
// with the spectrum H (512 entries) as walk_preamble_fft's window pass does:
// c = 512 * IDFT-normalised correlation, FP32 tier (f32) or FP64 pass.
int ofdm_devtest_corr(int f32, const double* x, const double* H, double* c, long nw, hipStream_t s)
{
    if (nw <= 0) return 0;
    const double2* tw = device_twiddles(9);
    if (!tw) return -1;
    const double2* xx = reinterpret_cast<const double2*>(x);
    const double2* hh = reinterpret_cast<const double2*>(H);
    double2* cc = reinterpret_cast<double2*>(c);
    if (f32)
        hipLaunchKernelGGL(corr_kernel<true>, dim3((unsigned)nw), dim3(64), 0, s, xx, hh, cc, tw);
    else
        hipLaunchKernelGGL(corr_kernel<false>, dim3((unsigned)nw), dim3(64), 0, s, xx, hh, cc, tw);
    return (int)hipGetLastError();
}

// the context's threshold scan: out = 3 thresholds + verdict (4 doubles)
int ofdm_devtest_tau_scan(int k, double* out, hipStream_t s)
{
    if (k != 2 && k != 4) return -1;
    hipLaunchKernelGGL(tau_scan_kernel, dim3(1), dim3(256), 0, s, k, out);
    return (int)hipGetLastError();
}

int ofdm_devtest_decide(int k, const double* z, const double* tau, uint8_t* sel, uint8_t* thr, long n,
                        hipStream_t s)
{
    if (k != 2 && k != 4) return -1;
    if (n <= 0) return 0;
    const dim3 grid((unsigned)((n + 255) / 256));
    const double2* zz = reinterpret_cast<const double2*>(z);
    if (k == 2)
        hipLaunchKernelGGL(decide_kernel<2>, grid, dim3(256), 0, s, zz, tau, sel, thr, n);
    else
        hipLaunchKernelGGL(decide_kernel<4>, grid, dim3(256), 0, s, zz, tau, sel, thr, n);
    return (int)hipGetLastError();
}

int ofdm_devtest_emit_words(int k, const unsigned* bits, unsigned* words, int nwaves, hipStream_t s)
{
    if (k != 2 && k != 4) return -1;
    if (nwaves <= 0) return 0;
    if (k == 2)
        hipLaunchKernelGGL(emit_words_kernel<2>, dim3(nwaves), dim3(64), 0, s, bits, words);
    else
        hipLaunchKernelGGL(emit_words_kernel<4>, dim3(nwaves), dim3(64), 0, s, bits, words);
    return (int)hipGetLastError();
}

int ofdm_devtest_atan2(const double* y, const double* x, double* out, long n, hipStream_t s)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(atan2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, x, out, n);
    return (int)hipGetLastError();
}

int ofdm_devtest_cp_phase(const double* acc, const double* rot, double* out, long n, hipStream_t s)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(cp_phase_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const double2*>(acc), reinterpret_cast<const double2*>(rot), out, n);
    return (int)hipGetLastError();
}

// The pilot windows' first maxima of nspec spectra of S bins (complex pairs)
// with borders[P + 2] each, 0 <= borders <= S (the caller's check): by the
// plain and by the screened helper, P + 1 ints per spectrum each, with a
// workgroup of nt = 128 or 256 threads. -1 for another nt or a bad size.
int ofdm_devtest_window_argmax(int nt, const double* spec, const int* borders, int P, int S, int nspec, int* plain,
                               int* screened, hipStream_t s)
{
    if (nspec <= 0) return 0;
    if (P < 1 || S < 1) return -1;
    const size_t shm = sizeof(double2) * (size_t)S + sizeof(int) * 2 * (size_t)(P + 1);
    if (shm > 64 * 1024) return -1;
    const double2* sp = reinterpret_cast<const double2*>(spec);
    if (nt == 128)
        hipLaunchKernelGGL(window_argmax_kernel<128>, dim3(nspec), dim3(128), shm, s, sp, borders, P, S, plain, screened);
    else if (nt == 256)
        hipLaunchKernelGGL(window_argmax_kernel<256>, dim3(nspec), dim3(256), shm, s, sp, borders, P, S, plain, screened);
    else
        return -1;
    return (int)hipGetLastError();
}

// unwrap_scan<nt, wave> on nseq rows of ph. Returns -1 for an instantiation
// that does not exist or a stride that cannot hold 4 * nt + 1 entries; the
// caller keeps every len[b] within 1 .. 4 * nt + 1.
int ofdm_devtest_unwrap(int nt, int wave, double* ph, const int* len, int nseq, long stride, hipStream_t s)
{
    if (nseq <= 0) return 0;
    if (stride < 4L * nt + 1) return -1;
    if (wave) return nt == 64 ? launch_unwrap<64, true>(ph, len, nseq, stride, s) : -1;
    switch (nt) {
    case 8: return launch_unwrap<8, false>(ph, len, nseq, stride, s);
    case 16: return launch_unwrap<16, false>(ph, len, nseq, stride, s);
    case 64: return launch_unwrap<64, false>(ph, len, nseq, stride, s);
    case 128: return launch_unwrap<128, false>(ph, len, nseq, stride, s);
    case 512: return launch_unwrap<512, false>(ph, len, nseq, stride, s);
    default: return -1;
    }
}

}  // extern "C"
