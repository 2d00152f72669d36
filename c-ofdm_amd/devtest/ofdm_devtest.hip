// ofdm_devtest.hip — test-only launchers for two device primitives of the rx
// sync front end that no C-ABI entry reaches with chosen arguments:
// atan2_fast / cp_phase (ofdm_fft.hpp) and unwrap_scan (ofdm_syncdev.hpp).
// Built into lib/libofdm_devtest.so, a library of its own: nothing here is
// linked into libofdm_mi355x.so. Every launcher takes device pointers and a
// stream, launches one kernel and returns the launch's hipError_t.
#include <hip/hip_runtime.h>

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

}  // namespace

extern "C" {

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
