// ofdm_csi.hip — the frequency-selective channel path of include/ofdm_mi355x.h
// ("frequency-selective channels"): the least-squares per-carrier channel
// estimate from the preamble form and the max-log demapper whose LLRs carry a
// per-carrier weight. DESIGN.md "Frequency-selective channels" has the
// structure, the LDS layout and the measurements.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "ofdm_csi.hpp"
#include "ofdm_dev.hpp"
#include "ofdm_fft.hpp"
#include "ofdm_syncdev.hpp"

namespace ofdm {
namespace {

// ========================================================================
// Least-squares estimate: FFT_FORM::read of the preamble form (phys over its
// pilots, coef against symbol 0: chan_kernel's points) on all D carriers of
// every preamble symbol, divided by the preamble's own points and averaged
// over the symbols; an optional moving mean over up to 2w+1 carriers that
// stays on its side of DC. One workgroup per frame. phys is known only after
// the last symbol, so est[] accumulates F_s / coef_s / m and 1/(phys*npr) is
// applied on the way out (coef_s, a ratio of two pilots, needs no phys).
// ========================================================================
template <int LOGN>
__global__ void __launch_bounds__((1 << LOGN) / 8) chan_ls_kernel(ChanLsArgs a)
{
    using FS = FftShape<LOGN>;
    constexpr int N = FS::N, T = FS::T;
    extern __shared__ double2 smem[];
    double2* lds_tw = smem;
    double2* fftb = lds_tw + TwLds<LOGN>::SIZE;   // N
    double2* pil = fftb + N;                       // npr * P raw pilot bins
    double2* est = pil + a.npr * a.P;              // D: sum over the symbols of F / coef / m
    double2* red = est + a.D;                      // 16: block_sum2's wave sums
    const int t = threadIdx.x;
    const long f = blockIdx.x;
    const double2* x = a.x + f * a.frame_stride;
    const int L = N + a.cp, D = a.D, half = a.D / 2;
    load_twiddles<LOGN>(a.tab.tw, lds_tw, t, T);
    __syncthreads();
    for (int s = 0; s < a.npr; ++s) {
        double2 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = x[(long)s * L + a.cp + t + T * i];
        fft_block<LOGN, -1>(v, t, lds_tw, fftb);
        for (int j = t; j < a.P; j += T) pil[s * a.P + j] = fftb[lds_swz(a.tab.pilot_bin[j])];
        // thread t owns est[t + T*u] through every symbol; pil[0..P) (symbol
        // 0's pilots) is visible from the barrier that ended symbol 0
        for (int i = t; i < D; i += T) {
            const int pb = a.tab.pilot_bin[a.tab.data_slot[i]];
            const double2 ps = fftb[lds_swz(pb)];
            const double2 p0 = s == 0 ? ps : pil[a.tab.data_slot[i]];
            const double2 coef = cdiv_exact(ps, p0);
            const double2 q = cdiv_exact(cdiv_exact(fftb[lds_swz(a.tab.data_bin[i])], coef), a.mod_pre[(long)s * D + i]);
            est[i] = s == 0 ? q : cadd(est[i], q);
        }
        __syncthreads();
    }
    // phys (Frame.cpp:76-80), parallel sum
    double acc = 0.0;
    for (int i = t; i < a.npr * a.P; i += T) acc += hypot(pil[i].x, pil[i].y);
    acc = block_sum2<T>(make_double2(acc, 0.0), red).x;
    const double phys = acc / ((double)(a.P * a.npr) * a.pilot_ampl);
    const double inv = 1.0 / (phys * (double)a.npr);
    const int w = a.smooth;
    double2* chan = a.chan_out ? a.chan_out + f * a.chan_stride : nullptr;
    double* csi = a.csi_out ? a.csi_out + f * a.csi_stride : nullptr;
    for (int i = t; i < D; i += T) {
        double2 h = est[i];
        if (w > 0) {
            const int lo = i < half ? 0 : half, hi = i < half ? half : D;
            const int c0 = i - w > lo ? i - w : lo, c1 = i + w < hi - 1 ? i + w : hi - 1;
            h = est[c0];
            for (int c = c0 + 1; c <= c1; ++c) h = cadd(h, est[c]);
            const double n = (double)(c1 - c0 + 1);
            h = make_double2(h.x / n, h.y / n);
        }
        h = make_double2(h.x * inv, h.y * inv);
        if (chan) chan[i] = h;
        if (csi) csi[i] = h.x * h.x + h.y * h.y;
    }
}

template <int LOGN>
hipError_t chan_ls_launch_n(const ChanLsArgs& a, hipStream_t st)
{
    using FS = FftShape<LOGN>;
    const size_t shm = chan_ls_lds_bytes(LOGN, a.npr, a.D, a.P);
    if (shm > CSI_LDS_MAX) return hipErrorInvalidValue;
    lds_opt_in((const void*)chan_ls_kernel<LOGN>, (int)CSI_LDS_MAX);
    hipLaunchKernelGGL(chan_ls_kernel<LOGN>, dim3((unsigned)a.nframes), dim3(FS::T), shm, st, a);
    return hipGetLastError();
}

// ========================================================================
// soft_demap_kernel (ofdm_kernels.hip) with a scale per point: s = scale *
// frame_scale[f] * csi[f][c], c the point's carrier. A work item is a run of
// tiles_per_item consecutive tiles (256 x 4 points each) of one frame, so the
// frame (and with it the weight vector and the frame scale) is uniform over
// the workgroup and the carrier of a lane's next point is a counter: c += 256
// mod D, wrapped once. The D weights of a frame are read num_symb times: with
// the frame's tiles on one workgroup they come from memory once and from that
// CU's cache after that. (One tile per item, the first version, dealt the
// tiles of a frame to the 8 XCDs round-robin, and every XCD's L2 fetched every
// frame's vector: DESIGN.md.) Where D divides the tile, a lane's four carriers
// are the same in every tile and it loads its weights once. The launch splits
// a frame over several items only where there are fewer frames than resident
// workgroups. A point or a weight that is not usable (non-finite component;
// weight not finite and > 0) writes k exact zeros instead.
// ========================================================================
template <int FMT>
__global__ void __launch_bounds__(256) soft_demap_csi_kernel(SoftCsiArgs a, int items_per_frame, int tiles_per_item,
                                                             int step)
{
    constexpr int PT = 4, TILE = 256 * PT, ESZ = FMT == LLR_F32 ? 4 : 1;
    __shared__ uint4 stage16[TILE * 8 * ESZ / 16];
    char* stage = reinterpret_cast<char*>(stage16);
    const int t = threadIdx.x, k = a.k;
    const int m = 1 << (k / 2);
    const double s1 = k == 1 ? 0.0 : 1.0 / (2.0 / (m - 1));
    SoftScale sq = soft_scale(k, 1.0);  // sq.c: LLR per unit of scale
    const double unit = sq.c;
    const int gsz = k * ESZ;  // bytes per point
    const int tiles_per_frame = (a.npts + TILE - 1) / TILE;
    const bool same_carriers = TILE % a.D == 0;
    const long nitems = a.nframes * items_per_frame;
    for (long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const long f = item / items_per_frame;
        const int tile0 = (int)(item - f * items_per_frame) * tiles_per_item;
        const int tile1 = tile0 + tiles_per_item < tiles_per_frame ? tile0 + tiles_per_item : tiles_per_frame;
        const double* wt = a.csi + f * a.csi_stride;
        const double sf = a.frame_scale ? a.scale * a.frame_scale[f] : a.scale;
        double wv[PT];
        for (int tile = tile0; tile < tile1; ++tile) {
            const int p0 = tile * TILE;
            const int np = a.npts - p0 < TILE ? a.npts - p0 : TILE;  // points of this tile
            const double2* pts = a.pts + f * (long)a.npts + p0;
            double2 z[PT];
#pragma unroll
            for (int i = 0; i < PT; ++i)
                z[i] = t + 256 * i < np ? load_nt(pts + t + 256 * i) : make_double2(0.0, 0.0);
            // D | TILE: a lane's four carriers are the same in every tile, its weights are loaded once per item
            if (!same_carriers || tile == tile0) {
                int c = (p0 + t) % a.D;
#pragma unroll
                for (int i = 0; i < PT; ++i) {
                    wv[i] = wt[c];  // c < D whatever the tile's point count
                    c += step;
                    c = c >= a.D ? c - a.D : c;
                }
            }
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                if (t + 256 * i >= np) continue;
                char* dst = stage + (t + 256 * i) * gsz;
                const bool ok = __builtin_isfinite(z[i].x) && __builtin_isfinite(z[i].y) && __builtin_isfinite(wv[i]) &&
                                wv[i] > 0.0;
                if (ok) {
                    sq.c = unit * (sf * wv[i]);
                    soft_emit(z[i], k, s1, sq, FMT, dst, true);
                } else if constexpr (FMT == LLR_F32) {
                    for (int b = 0; b < k; ++b) reinterpret_cast<float*>(dst)[b] = 0.0f;
                } else {
                    for (int b = 0; b < k; ++b) dst[b] = 0;
                }
            }
            __syncthreads();
            char* dst = static_cast<char*>(a.out) + (f * (long)a.npts + p0) * gsz;
            const bool vec = ((uintptr_t)dst & 15) == 0;
            const int nb = np * gsz;  // bytes of this tile's output
            const int n16 = vec ? nb >> 4 : 0;
            for (int q = t; q < n16; q += 256) reinterpret_cast<uint4*>(dst)[q] = stage16[q];
            if constexpr (FMT == LLR_F32) {
                for (int e = n16 * 4 + t; e < nb / 4; e += 256)
                    reinterpret_cast<float*>(dst)[e] = reinterpret_cast<const float*>(stage)[e];
            } else {
                for (int e = n16 * 16 + t; e < nb; e += 256) dst[e] = stage[e];
            }
            __syncthreads();  // the stage is rewritten by the next tile
        }
    }
}

// Compute units of the current device (cached per device).
int csi_num_cus()
{
    static int cache[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!cache[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cache[dev] = n;
    }
    return cache[dev];
}

}  // namespace

size_t chan_ls_lds_bytes(int logn, int npr, int D, int P)
{
    const size_t n = (size_t)1 << logn;
    return sizeof(double2) * (n / 64 + 64 + n + (size_t)npr * (size_t)P + (size_t)D + 16);
}

hipError_t launch_chan_ls(int logn, const ChanLsArgs& a, hipStream_t st)
{
    if (a.nframes <= 0) return hipSuccess;
    if (a.nframes > 0x7fffffffL) return hipErrorInvalidValue;
    switch (logn) {
        case 6: return chan_ls_launch_n<6>(a, st);
        case 7: return chan_ls_launch_n<7>(a, st);
        case 8: return chan_ls_launch_n<8>(a, st);
        case 9: return chan_ls_launch_n<9>(a, st);
        case 10: return chan_ls_launch_n<10>(a, st);
        case 11: return chan_ls_launch_n<11>(a, st);
        case 12: return chan_ls_launch_n<12>(a, st);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_soft_demap_csi(const SoftCsiArgs& a, hipStream_t st)
{
    if (a.nframes <= 0 || a.npts <= 0) return hipSuccess;
    const long tpf = ((long)a.npts + 1023) / 1024;
    const long cap = 8L * csi_num_cus();  // grid-stride: 2048 resident threads per CU, as soft_demap_kernel
    // whole frames per item where the frames alone fill the device, else as few items per frame as do
    long ipf = (cap + a.nframes - 1) / a.nframes;
    ipf = ipf < tpf ? ipf : tpf;
    const long tpi = (tpf + ipf - 1) / ipf;
    ipf = (tpf + tpi - 1) / tpi;
    const long nitems = a.nframes * ipf;
    const unsigned grid = (unsigned)(nitems < cap ? nitems : cap);
    const int step = 256 % a.D;
    if (a.fmt == LLR_F32)
        hipLaunchKernelGGL(soft_demap_csi_kernel<LLR_F32>, dim3(grid), dim3(256), 0, st, a, (int)ipf, (int)tpi, step);
    else
        hipLaunchKernelGGL(soft_demap_csi_kernel<LLR_I8>, dim3(grid), dim3(256), 0, st, a, (int)ipf, (int)tpi, step);
    return hipGetLastError();
}

}  // namespace ofdm
