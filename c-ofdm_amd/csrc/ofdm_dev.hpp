// ofdm_dev.hpp — device helpers shared by the rx kernels (ofdm_kernels.hip)
// and the fused stream decode (ofdm_sync.hip): the demod decision, output
// byte packing and non-temporal 16-B accesses.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <mutex>
#include <set>
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
