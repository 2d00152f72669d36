// ofdm_devtest.hip — test-only launchers for device primitives that no C-ABI
// entry reaches with chosen arguments: atan2_fast / cp_phase (ofdm_fft.hpp),
// unwrap_scan (ofdm_syncdev.hpp), and the rx emit's fast path (ofdm_dev.hpp):
// the threshold scan, the decision by thresholds beside decide_select, and
// the in-wave assembly of output words.
// Built into lib/libofdm_devtest.so, a library of its own: nothing here is
// linked into libofdm_mi355x.so. Every launcher takes device pointers and a
// stream, launches one kernel and returns the launch's hipError_t.
#include <hip/hip_runtime.h>

#include "../csrc/ofdm_dev.hpp"
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

}  // namespace

extern "C" {

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
