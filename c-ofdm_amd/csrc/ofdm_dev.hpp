// ofdm_dev.hpp — device helpers shared by the rx kernels (ofdm_kernels.hip)
// and the fused stream decode (ofdm_sync.hip): the demod decision, output
// byte packing and non-temporal 16-B accesses.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>

#include "ofdm_fft.hpp"

namespace ofdm {

// Host side: opt a kernel into `bytes` of dynamic LDS once per (kernel,
// device). The launch helpers run on any host thread (one context per thread,
// or two contexts on two streams) and on any device of the process.
inline void lds_opt_in(const void* fn, int bytes)
{
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> g(mu);
    if (done.insert({fn, dev}).second)
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// Modulation::demod decision for one point (modulation.cpp:62-84): BPSK
// re+im > 0; QAM clamp to [-1,1] then uint8((v+1)*str_size_1 + 0.5) per axis,
// idx = re | im*str_size. Separate roundings (no FMA) as on x86-64.
// The clamp is v_max/v_min: equal to the reference's compare chain for every
// non-NaN value; a NaN (degenerate all-zero pilots) decides 0 either way
// (chain: cvt(NaN) = 0; min/max: clamps to -1, then uint8(0.5) = 0).
// decide() as a select (no branch on k): the same value for every k.
__device__ __forceinline__ int decide_select(double2 z, int k, double s1, int m)
{
    const double re = __builtin_fmin(__builtin_fmax(z.x, -1.0), 1.0);
    const double im = __builtin_fmin(__builtin_fmax(z.y, -1.0), 1.0);
    const int ire = (uint8_t)(int)add_rn(mul_rn(add_rn(re, 1.0), s1), 0.5);
    const int iim = (uint8_t)(int)add_rn(mul_rn(add_rn(im, 1.0), s1), 0.5);
    const int qam = (ire | (iim * m)) & 0xff;
    const int bpsk = (z.x + z.y) > 0.0;
    return k == 1 ? bpsk : qam;
}

// ---- the QAM decision as threshold compares (the rx emit's fast path).
// decide_select's per-axis level is a composition of monotone steps (clamp,
// rounded add, rounded multiply by s1 > 0, rounded add, truncation), so it is
// a monotone step function of the coordinate: the level equals the number of
// thresholds tau_1 < tau_2 < ... the coordinate has reached. The tau are
// particular doubles, not the nominal cell edges (QPSK: tau_1 is just below 0,
// because x + 1 rounds to 1 there); decide_tau_scan finds them by evaluating
// decide_select itself. A NaN reaches no threshold: level 0, as decide_select.
// The product runs K = 2 only: the K = 4 forms of axis_tau, emit_collects and
// emit_words below are the record of the 16-QAM emit that measured no gain
// (DESIGN section 4), reached through the devtest library and tested there,
// so that the experiment can be repeated without rewriting them.
constexpr int DEC_TAU_MAX = 3;  // m - 1 thresholds per axis, m <= 4 (k = 2, 4)

// Level of one axis for k in {2, 4}: the bits come from the nested compare
// masks (16-QAM: high bit [x >= tau_2], low bit the parity of the three).
template <int K>
__device__ __forceinline__ unsigned axis_tau(double x, const double (&tau)[DEC_TAU_MAX])
{
    static_assert(K == 2 || K == 4, "thresholds cover QPSK and 16-QAM");
    if constexpr (K == 2) {
        return x >= tau[0] ? 1u : 0u;
    } else {
        const bool c0 = x >= tau[0], c1 = x >= tau[1], c2 = x >= tau[2];
        return (c1 ? 2u : 0u) | ((c0 != c1) != c2 ? 1u : 0u);
    }
}

// decide_select(z, K, ...) from thresholds: re | im * m, K bits.
template <int K>
__device__ __forceinline__ unsigned decide_tau(double2 z, const double (&tau)[DEC_TAU_MAX])
{
    return axis_tau<K>(z.x, tau) | (axis_tau<K>(z.y, tau) << (K / 2));
}

// Order-preserving map between doubles and signed 64-bit keys (-0 < +0,
// adjacent doubles are adjacent keys), NaNs excluded.
__device__ __forceinline__ long long dbl_key(double x)
{
    const long long b = __double_as_longlong(x);
    return b ^ ((b >> 63) & 0x7fffffffffffffffLL);
}
__device__ __forceinline__ double key_dbl(long long k)
{
    return __longlong_as_double(k ^ ((k >> 63) & 0x7fffffffffffffffLL));
}

// The thresholds of k in {2, 4}, found on the device from decide_select
// itself. One workgroup of 256 threads; out[0 .. DEC_TAU_MAX-1] = tau (unused
// entries +inf), out[DEC_TAU_MAX] = 1.0 if every check below held, else 0.0
// (the context then does not offer the fast path):
//   * thread 0 bisects, in key order, for the smallest double whose level is
//     >= j between nominal edge -+ 1/4 (levels j-1 and j there);
//   * every thread then compares decide_select with the threshold count on
//     the 2048 doubles around each tau (monotone across the step), on 4096
//     points of a sweep over [-1.5, 1.5], and on the special values
//     (+-0, +-1 and neighbours, +-2, +-inf, NaN), both axes.
// lds: DEC_TAU_MAX + 1 doubles.
__device__ __forceinline__ void decide_tau_scan(int k, double* __restrict__ out, double* lds)
{
    const int m = 1 << (k / 2);
    const double s1 = 1.0 / (2.0 / (m - 1));  // rx_kernel's expression
    auto level = [&](double x) { return decide_select(make_double2(x, -1.0), k, s1, m) & (m - 1); };
    const int t = threadIdx.x;
    if (t == 0) {
        bool ok = true;
        for (int j = 1; j < DEC_TAU_MAX + 1; ++j) {
            if (j >= m) {
                lds[j - 1] = __longlong_as_double(0x7ff0000000000000LL);
                continue;
            }
            const double edge = -1.0 + (double)(2 * j - 1) / (double)(m - 1);
            long long lo = dbl_key(edge - 0.25), hi = dbl_key(edge + 0.25);
            ok = ok && level(key_dbl(lo)) == j - 1 && level(key_dbl(hi)) == j;
            while (hi - lo > 1) {  // level(lo) < j <= level(hi)
                const long long mid = lo + (hi - lo) / 2;
                if (level(key_dbl(mid)) >= j)
                    hi = mid;
                else
                    lo = mid;
            }
            lds[j - 1] = key_dbl(hi);
        }
        lds[DEC_TAU_MAX] = ok ? 1.0 : 0.0;
    }
    __syncthreads();
    double tau[DEC_TAU_MAX];
    for (int j = 0; j < DEC_TAU_MAX; ++j) tau[j] = lds[j];
    bool ok = lds[DEC_TAU_MAX] != 0.0;
    auto same = [&](double x, double y) {
        const double2 z = make_double2(x, y);
        const unsigned want = (unsigned)decide_select(z, k, s1, m);
        return want == (k == 2 ? decide_tau<2>(z, tau) : decide_tau<4>(z, tau));
    };
    for (int j = 0; j < m - 1; ++j) {
        const long long c = dbl_key(tau[j]);
        int prev = level(key_dbl(c - 1024 + t * 8 - 1));
        for (int e = 0; e < 8; ++e) {
            const double x = key_dbl(c - 1024 + t * 8 + e);
            const int lv = level(x);
            ok = ok && lv >= prev && same(x, -x) && same(-x, x);
            prev = lv;
        }
    }
    for (int i = t; i < 4096; i += 256) {
        const double x = -1.5 + 3.0 * (double)i / 4095.0;
        ok = ok && same(x, 0.3 - x) && level(x) <= level(x + 3.0 / 4095.0);
    }
    const double inf = __longlong_as_double(0x7ff0000000000000LL), qnan = __longlong_as_double(0x7ff8000000000000LL);
    const double sp[16] = {0.0, -0.0, 1.0, -1.0, 1.0 + DBL_EPSILON, 1.0 - DBL_EPSILON / 2, -1.0 - DBL_EPSILON,
                           -1.0 + DBL_EPSILON / 2, 2.0, -2.0, inf, -inf, qnan, -qnan, 0.5, -0.5};
    ok = ok && same(sp[t & 15], sp[(t >> 4) & 15]);
    const int all = __syncthreads_and(ok ? 1 : 0);
    if (t == 0) {
        for (int j = 0; j < DEC_TAU_MAX; ++j) out[j] = tau[j];
        out[DEC_TAU_MAX] = all ? 1.0 : 0.0;
    }
}

// One symbol's output words, assembled inside a wave (whole waves, uniform
// control flow). Lane l holds in `bits` its K-bit decisions of the symbol's
// four 64-carrier groups (carriers w0 + T*g + l), group g in byte g. An output
// byte takes LPB = 8/K consecutive carriers, MSB first (pack_word's order):
// each lane shifts its decisions to their place in the byte and the LPB lanes
// of a byte are OR-ed by quad permutations, which leaves in each of them
// v: byte g = output byte l/LPB of group g. Four consecutive bytes of one
// group (an output word) then sit in byte g of four neighbouring lane cells
// of one 16-lane row: each lane moves the byte of "its" group(s) to the
// byte's place in the word, and the last cell of the four (the collecting
// lanes, emit_collects) ORs the cells below it in by row shifts.
//   K = 2: w[0] = word l/16 of group l & 3                  (lanes 12..15 of a row)
//   K = 4: w[h] = word l/8 of group (l & 1) + 2h, h = 0, 1  (lanes 6, 7, 14, 15)
// Values in the other lanes are partial.
template <int K>
__device__ __forceinline__ bool emit_collects(int lane)
{
    return ((lane / (8 / K)) & 3) == 3;
}

template <int K>
__device__ __forceinline__ void emit_words(unsigned bits, int lane, unsigned (&w)[K / 2])
{
    constexpr int LPB = 8 / K;
    auto dpp = [](unsigned x, auto ctrl) {  // lanes without a source read 0
        return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, decltype(ctrl)::value, 0xf, 0xf, true);
    };
    const int r = lane & (LPB - 1);
    unsigned v = bits << (K * (LPB - 1 - r));
    v |= dpp(v, std::integral_constant<int, 0xB1>{});  // quad_perm [1,0,3,2]
    if constexpr (LPB == 4) v |= dpp(v, std::integral_constant<int, 0x4E>{});  // quad_perm [2,3,0,1]
    const int q = (lane / LPB) & 3;  // this cell's byte within its output words
#pragma unroll
    for (int h = 0; h < K / 2; ++h) {
        const int g = r + LPB * h;
        const unsigned b = ((v >> (8 * g)) & 0xffu) << (8 * q);
        w[h] = b | dpp(b, std::integral_constant<int, 0x110 + LPB>{})       // row_shr: lane i reads lane i - n
                 | dpp(b, std::integral_constant<int, 0x110 + 2 * LPB>{})
                 | dpp(b, std::integral_constant<int, 0x110 + 3 * LPB>{});
    }
}

// ---- soft decisions: max-log LLRs of the reference's constellation
// (modulation.cpp:4-36; natural binary per axis, symbol = col | row*m).
//   L_b = s * ( min_{c: bit_b(c)=1} |z-c|^2 - min_{c: bit_b(c)=0} |z-c|^2 ),
// from the equalised point BEFORE demod's clamp; L_b > 0 means bit 0; bits MSB
// first (row = imaginary axis first, then col = real axis), the order
// bit_stream_converter emits. QAM is separable: per axis, in level units
// u = (x+1)(m-1)/2 (levels at 0..m-1), the nearest level j (demod's own index)
// is the same-bit minimum and the opposite-bit minimum is the nearer edge
// level jo of the two adjacent blocks of 2^(h-1-b) levels, so
//   min_opp - min_same = (u-jo)^2 - (u-j)^2 = (j-jo)(2u-j-jo)  [level units^2]
// with exact integer factors: one rounding in u, no cancellation of squares.
enum { LLR_F32 = 0, LLR_I8 = 1 };

// Per-frame constants of the demapper: c = s/h1^2 (QAM, h1 = (m-1)/2: level
// units^2 -> LLR) or -2*sqrt(2)*s (BPSK: L_0 = c*(re+im), constellation
// (+-1+-j)/sqrt(2) on the diagonal, modulation.cpp:28-30).
struct SoftScale {
    double c, h1;
    int h;  // bits per axis (0: BPSK)
};

__device__ __forceinline__ SoftScale soft_scale(int k, double s)
{
    SoftScale q;
    q.h = k >> 1;
    q.h1 = (double)((1 << q.h) - 1) * 0.5;
    q.c = k == 1 ? -2.8284271247461903 * s : s / (q.h1 * q.h1);
    return q;
}

// One axis: L[b], b < H, for bit b (MSB first) of the axis' level index. H is
// static, so every shift below is an immediate; H = 1 (QPSK) collapses to
// L = -c*x (levels -1, +1: (x+1)^2 - (x-1)^2 = 4x, c = 4s).
template <int H>
__device__ __forceinline__ void soft_axis(double x, double s1, const SoftScale& q, double (&L)[4])
{
#pragma unroll
    for (int b = 0; b < 4; ++b) L[b] = 0.0;
    if constexpr (H == 1) {
        L[0] = -(q.c * x);
    } else if constexpr (H == 2) {
        // 16-QAM: with t = u - 3/2 = 3x/2 the two bits are clamps of t, no
        // index needed: MSB (blocks {0,1}|{2,3}) 2*clamp(t,-1,1) - 4t,
        // LSB (alternating levels) 4*clamp(t,-1/2,1/2) - 2t
        const double t = 1.5 * x;
        const double t1 = __builtin_fmin(__builtin_fmax(t, -1.0), 1.0);
        const double th = __builtin_fmin(__builtin_fmax(t, -0.5), 0.5);
        L[0] = q.c * __builtin_fma(-4.0, t, t1 + t1);
        L[1] = q.c * __builtin_fma(4.0, th, -(t + t));
    } else if constexpr (H > 2) {
        const double xc =__builtin_fmin(__builtin_fmax(x, -1.0), 1.0);
        const int j = (uint8_t)(int)add_rn(mul_rn(add_rn(xc, 1.0), s1), 0.5);  // decide()'s index
        const double h2 = q.h1 + q.h1;
        const double u2 = __builtin_fma(x, h2, h2);  // 2u = 2(x+1)h1, not clamped
        // u2 < n for an integer n is floor(u2) < n; the truncation equals the
        // floor wherever it is used (blk > 0: x > -1, u2 > 0)
        const int fu2 = (int)u2;
#pragma unroll
        for (int b = 0; b < H; ++b) {
            const int sh = H - 1 - b;
            const int blk = j >> sh;
            const int lo = (blk << sh) - 1, hi = (blk + 1) << sh;  // edge levels of the adjacent blocks
            const bool use_lo = blk > 0 && ((hi >> H) != 0 || fu2 < lo + hi);
            const int jo = use_lo ? lo : hi;
            const double v = q.c * ((double)(j - jo) * (u2 - (double)(j + jo)));
            L[b] = (blk & 1) ? -v : v;
        }
    }
}

__device__ __forceinline__ int llr_i8(double L)
{
    return (int)__builtin_fmin(__builtin_fmax(__builtin_rint(L), -127.0), 127.0);  // rint: half to even
}

// The k LLRs of point z to dst (element size 4 or 1 B). vec: dst is aligned
// to the point's whole k-element group (or 16 B), so the group goes out in
// 2- to 16-B pieces; otherwise element by element.
template <int H, int FMT>
__device__ __forceinline__ void soft_emit_t(double2 z, double s1, const SoftScale& q, void* dst, bool vec)
{
    constexpr int k = H ? 2 * H : 1, h = H, fmt = FMT;
    if (k == 1) {
        const double L = q.c * (z.x + z.y);
        if (fmt == LLR_F32)
            *reinterpret_cast<float*>(dst) = (float)L;
        else
            *reinterpret_cast<int8_t*>(dst) = (int8_t)llr_i8(L);
        return;
    }
    double Lr[4], Lc[4];
    soft_axis<H>(z.y, s1, q, Lr);  // row bits first (symbol = col | row*m, MSB first)
    soft_axis<H>(z.x, s1, q, Lc);
    if (fmt == LLR_F32) {
        float fr[4], fc[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            fr[b] = (float)Lr[b];
            fc[b] = (float)Lc[b];
        }
        float* o = reinterpret_cast<float*>(dst);
        if (!vec) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b < h) {
                    o[b] = fr[b];
                    o[h + b] = fc[b];
                }
        } else if (h == 1) {
            *reinterpret_cast<float2*>(o) = make_float2(fr[0], fc[0]);
        } else if (h == 2) {
            *reinterpret_cast<float4*>(o) = make_float4(fr[0], fr[1], fc[0], fc[1]);
        } else if (h == 3) {
            float2* o2 = reinterpret_cast<float2*>(o);
            o2[0] = make_float2(fr[0], fr[1]);
            o2[1] = make_float2(fr[2], fc[0]);
            o2[2] = make_float2(fc[1], fc[2]);
        } else {
            float4* o4 = reinterpret_cast<float4*>(o);
            o4[0] = make_float4(fr[0], fr[1], fr[2], fr[3]);
            o4[1] = make_float4(fc[0], fc[1], fc[2], fc[3]);
        }
    } else {
        uint32_t rw = 0, cw = 0;  // byte b = bit b's LLR (absent bits: 0)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            rw |= (uint32_t)(llr_i8(Lr[b]) & 0xff) << (8 * b);
            cw |= (uint32_t)(llr_i8(Lc[b]) & 0xff) << (8 * b);
        }
        uint8_t* o = reinterpret_cast<uint8_t*>(dst);
        if (!vec) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b < h) {
                    o[b] = (uint8_t)(rw >> (8 * b));
                    o[h + b] = (uint8_t)(cw >> (8 * b));
                }
        } else if (h == 1) {
            *reinterpret_cast<uint16_t*>(o) = (uint16_t)(rw | (cw << 8));
        } else if (h == 2) {
            *reinterpret_cast<uint32_t*>(o) = rw | (cw << 16);
        } else if (h == 3) {
            uint16_t* o2 = reinterpret_cast<uint16_t*>(o);
            o2[0] = (uint16_t)rw;
            o2[1] = (uint16_t)((rw >> 16) | (cw << 8));
            o2[2] = (uint16_t)(cw >> 8);
        } else {
            *reinterpret_cast<uint2*>(o) = make_uint2(rw, cw);
        }
    }
}

// soft_emit_t for the launch's k and format: a uniform jump to the code
// compiled for them (static shifts, no dead bits held in registers).
__device__ __forceinline__ void soft_emit(double2 z, int k, double s1, const SoftScale& q, int fmt, void* dst,
                                          bool vec)
{
    switch ((k >> 1) | (fmt == LLR_F32 ? 0 : 8)) {
        case 0: soft_emit_t<0, LLR_F32>(z, s1, q, dst, vec); break;
        case 1: soft_emit_t<1, LLR_F32>(z, s1, q, dst, vec); break;
        case 2: soft_emit_t<2, LLR_F32>(z, s1, q, dst, vec); break;
        case 3: soft_emit_t<3, LLR_F32>(z, s1, q, dst, vec); break;
        case 4: soft_emit_t<4, LLR_F32>(z, s1, q, dst, vec); break;
        case 8: soft_emit_t<0, LLR_I8>(z, s1, q, dst, vec); break;
        case 9: soft_emit_t<1, LLR_I8>(z, s1, q, dst, vec); break;
        case 10: soft_emit_t<2, LLR_I8>(z, s1, q, dst, vec); break;
        case 11: soft_emit_t<3, LLR_I8>(z, s1, q, dst, vec); break;
        default: soft_emit_t<4, LLR_I8>(z, s1, q, dst, vec); break;
    }
}

// Four output bytes (one little-endian word) from 32/K consecutive K-bit
// decisions held one per byte in LDS (MSB-first within each byte, as
// bit_stream_converter(8, K, ...), modulation.cpp:90-125).
template <int K>
__device__ __forceinline__ uint32_t pack_word(const uint8_t* __restrict__ dec)
{
    constexpr int PER = 8 / K;  // decisions per output byte
    constexpr int NW = 8 / K;   // 32-bit LDS words holding the 32/K decisions (dec is 32/K-byte aligned)
    uint32_t d[NW];
    const uint32_t* d32 = reinterpret_cast<const uint32_t*>(dec);
#pragma unroll
    for (int i = 0; i < NW; ++i) d[i] = d32[i];
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        uint32_t byte = 0;
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int idx = b * PER + r;
            byte = (byte << K) | ((d[idx >> 2] >> (8 * (idx & 3))) & 0xffu);
        }
        word |= byte << (8 * b);
    }
    return word;
}

// Streams touched once (tx output, rx input, constellation output): non-temporal
// 16-B accesses, so a launch neither evicts the caches for nothing nor leaves
// gigabytes of dirty lines for the next launch to write back.
typedef double nt_double2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void store_nt(double2* p, double2 v)
{
    nt_double2 w = {v.x, v.y};
    __builtin_nontemporal_store(w, reinterpret_cast<nt_double2*>(p));
}

__device__ __forceinline__ double2 load_nt(const double2* p)
{
    const nt_double2 w = __builtin_nontemporal_load(reinterpret_cast<const nt_double2*>(p));
    return make_double2(w.x, w.y);
}

}  // namespace ofdm
