// ofdm_fec.hip — the channel code of include/ofdm_mi355x.h ("channel code"):
// the K=7 133/171 convolutional encoder with its 2/3 and 3/4 puncturings, and
// the soft-input Viterbi decoder (one wave64 per codeword, lane = trellis
// state). DESIGN.md "Channel code" has the structure and the measurements.
#include "ofdm_internal.hpp"

namespace ofdm {
namespace {

constexpr int ENC_THREADS = 256;
constexpr int DEC_THREADS = 64 * FEC_CW_PER_WG;

// Mother-stream index of transmitted bit n, and transmitted index of kept
// mother bit i (closed forms of the puncture table: nothing is searched).
__device__ inline long fec_mother_index(const FecRate& r, long n)
{
    const long q = n / r.kept;
    const int j = (int)(n - q * r.kept);
    return q * r.period + (j < 3 ? j : 5);
}

__device__ inline bool fec_tx_index(const FecRate& r, long i, long* n)
{
    const long q = i / r.period;
    const int j = (int)(i - q * r.period);
    *n = q * r.kept + __popc(r.mask & ((1u << j) - 1u));
    return (r.mask >> j) & 1u;
}

// ---------------------------------------------------------------- encoder
// One thread per output byte. Bit n of the byte is a parity over the seven
// inputs u_{t-6} .. u_t of its step t; the eight bits of a byte span at most
// 7 steps, so one 40-bit window of the info stream (5 bytes, zero outside
// [0, info_bits)) serves them all. With the newest input at bit 0 of the
// 7-bit field the generators are 0133 and 0171 bit-reversed: 0155 and 0117.
__global__ __launch_bounds__(ENC_THREADS) void fec_encode_kernel(FecEncArgs a)
{
    const size_t gid = (size_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    if (gid >= (size_t)a.ncw * (size_t)a.coded_stride) return;
    const long c = (long)(gid / (size_t)a.coded_stride);
    const long ob = (long)(gid - (size_t)c * (size_t)a.coded_stride);
    const long n0 = ob * 8;
    unsigned out = 0;
    if (n0 < a.coded_bits) {
        const FecRate r = fec_rate(a.rate);
        const uint8_t* in = a.info + (size_t)c * (size_t)a.info_stride;
        const long nbytes = (a.info_bits + 7) >> 3;
        const int rem = (int)(a.info_bits & 7);
        const long b0 = (fec_mother_index(r, n0) >> 1) - 6;  // first info bit of the window (may be < 0)
        const long byte0 = b0 >> 3;                          // floor
        const int sh = (int)(b0 - byte0 * 8);
        unsigned long long w = 0;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const long idx = byte0 + q;
            unsigned v = 0;
            if (idx >= 0 && idx < nbytes) {
                v = in[idx];
                if (rem && idx == nbytes - 1) v &= 0xffu << (8 - rem);
            }
            w = (w << 8) | v;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const long n = n0 + q;
            if (n < a.coded_bits) {
                const long i = fec_mother_index(r, n);
                const int j = (int)((i >> 1) - b0);  // 6..12: u_t is bit 39 - sh - j of w
                const unsigned f = (unsigned)(w >> (39 - sh - j)) & 0x7fu;
                const unsigned g = (i & 1) ? 0117u : 0155u;
                out |= (unsigned)(__popc(f & g) & 1) << (7 - q);
            }
        }
    }
    a.coded[(size_t)c * (size_t)a.coded_stride + (size_t)ob] = (uint8_t)out;
}

// ---------------------------------------------------------------- decoder
// Path metrics: int32 for int8 LLRs (|metric| <= 2*127*(2^20+6) < 2^29, and
// the states not yet reachable from state 0 start at -2^30, below every
// reachable metric for the six steps they exist), float for float LLRs.
template <class M> struct Metric;
template <> struct Metric<int> {
    using In = int8_t;
    static constexpr int unreachable = -(1 << 30);
    static __device__ int bits(int v) { return v; }
    static __device__ int from_bits(int b) { return b; }
};
template <> struct Metric<float> {
    using In = float;
    static constexpr float unreachable = -1e30f;
    static __device__ int bits(float v) { return __float_as_int(v); }
    static __device__ float from_bits(int b) { return __int_as_float(b); }
};

// The two LLRs of trellis step t (mother bits 2t, 2t+1), 0 where punctured or
// past the codeword. Across the lanes of a tile the kept positions are
// consecutive elements of llr: the loads of a tile cover whole cache lines.
template <class M>
__device__ inline void fec_load_step(const typename Metric<M>::In* llr, const FecRate& r, long t, long T, M* la, M* lb)
{
    *la = 0;
    *lb = 0;
    if (t < T) {
        long n;
        if (fec_tx_index(r, 2 * t, &n)) *la = (M)llr[n];
        if (fec_tx_index(r, 2 * t + 1, &n)) *lb = (M)llr[n];
    }
}

// One wave64 per codeword, lane s' = new trellis state. Both generators tap
// the oldest register bit, so the branch from predecessor p1 = p0 | 1 has the
// negated metric of the branch from p0 = (2 s') & 63: a step is
// bm = +-(L_A +- L_B) with lane-constant signs, pm[p0] + bm against
// pm[p1] - bm.
// Steps run in tiles of 64: lane l loads the LLR pair of step base + l
// (depunctured, zeros inserted) and writes its four possible branch metrics
// into the wave's LDS table; the step loop reads its lane's row at a constant
// offset (no puncture logic and no sign arithmetic inside the recursion) and
// each lane collects its own state's 64 decisions of the tile in one 64-bit
// word (bit = step), so the survivors leave as one 512-byte store per tile
// (LDS or the workspace): the words of the header's definition, transposed
// within a tile. The traceback walks the tiles backwards with the state in a
// scalar register, reading the decision of (step, state s) from lane s with
// v_readlane; decisions of steps >= T are stored as 0, which keeps state 0 in
// state 0, so it needs no partial tile. Waves never synchronise with each other.
template <class M, bool LDS_SURV, int GATHER>
__global__ __launch_bounds__(DEC_THREADS) void fec_decode_kernel(FecDecArgs a)
{
    extern __shared__ unsigned long long fec_surv_lds[];
    __shared__ __attribute__((aligned(8))) int xch[FEC_CW_PER_WG][64];
    __shared__ __attribute__((aligned(16))) int bmtab[FEC_CW_PER_WG][4 * 64];
    using In = typename Metric<M>::In;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long cw = (long)blockIdx.x * FEC_CW_PER_WG + w;
    if (cw >= a.ncw) return;
    const long T = a.info_bits + FEC_TAIL;
    const long Tpad = (T + 63) & ~63L;
    const FecRate r = fec_rate(a.rate);
    const In* llr = static_cast<const In*>(a.llr) + (size_t)cw * (size_t)a.llr_stride;
    unsigned long long* surv;
    if constexpr (LDS_SURV) surv = fec_surv_lds + (size_t)w * (size_t)Tpad;
    else surv = a.ws + (size_t)cw * (size_t)Tpad;

    // lane constants: encoder outputs of the branch p0 -> s' (input bit s' >> 5)
    const int p0 = (2 * lane) & 63;
    const unsigned reg0 = ((unsigned)(lane >> 5) << 6) | (unsigned)p0;
    const bool a0 = __popc(reg0 & 0133u) & 1, b0 = __popc(reg0 & 0171u) & 1;
    // bm is one of L_A + L_B, L_A - L_B, L_B - L_A, -L_A - L_B: the lane's row of the tile's table
    const int cls = a0 ? (b0 ? 3 : 2) : (b0 ? 1 : 0);
    M* tab = reinterpret_cast<M*>(bmtab[w]);
    const M* mybm = tab + cls * 64;

    M pm = lane == 0 ? (M)0 : Metric<M>::unreachable;
    M la, lb, nla, nlb;
    fec_load_step<M>(llr, r, lane, T, &la, &lb);
    for (long base = 0; base < Tpad; base += 64) {
        fec_load_step<M>(llr, r, base + 64 + lane, T, &nla, &nlb);  // next tile, in flight during this one
        // the tile's branch metrics, [class][step]: the step loop reads 4 addresses per
        // wave (a broadcast each), off the recursion's dependency chain. DS operations
        // of one wave complete in order, so the wave needs no barrier around the table.
        tab[lane] = la + lb;
        tab[64 + lane] = la - lb;
        tab[128 + lane] = lb - la;
        tab[192 + lane] = -la - lb;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        unsigned dec_lo = 0, dec_hi = 0;
#pragma unroll
        for (int tl = 0; tl < 64; ++tl) {
            const M bm = mybm[tl];
            M g0, g1;
            if constexpr (GATHER == 0) {
                g0 = Metric<M>::from_bits(__builtin_amdgcn_ds_bpermute(p0 * 4, Metric<M>::bits(pm)));
                g1 = Metric<M>::from_bits(__builtin_amdgcn_ds_bpermute(p0 * 4 + 4, Metric<M>::bits(pm)));
            } else {
                // DS operations of one wave complete in order: the pair read sees this step's writes
                volatile int* x1 = xch[w];
                x1[lane] = Metric<M>::bits(pm);
                __builtin_amdgcn_wave_barrier();
                const unsigned long long pr = *reinterpret_cast<volatile unsigned long long*>(&xch[w][p0]);
                __builtin_amdgcn_wave_barrier();
                g0 = Metric<M>::from_bits((int)(unsigned)pr);
                g1 = Metric<M>::from_bits((int)(unsigned)(pr >> 32));
            }
            const M c0 = g0 + bm, c1 = g1 - bm;
            const bool d = c1 > c0;  // a tie keeps j = 0
            pm = d ? c1 : c0;
            if (tl < 32) dec_lo |= (unsigned)d << tl;  // the lane's own decisions, bit = step in the tile
            else dec_hi |= (unsigned)d << (tl - 32);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the next tile's table is written after this tile's reads
        unsigned long long mydec = ((unsigned long long)dec_hi << 32) | dec_lo;
        if (T - base < 64) mydec &= (1ull << (T - base)) - 1ull;  // steps >= T: no decision, state 0 stays 0
        surv[base + lane] = mydec;
        la = nla;
        lb = nlb;
    }

    // traceback from state 0: info bit s >> 5, the step's decision from lane s's word
    const long nbytes = (a.info_bits + 7) >> 3;
    const int rem = (int)(a.info_bits & 7);
    uint8_t* out = a.out + (size_t)cw * (size_t)a.info_stride;
    const uint8_t* ref = a.ref ? a.ref + (size_t)cw * (size_t)a.info_stride : nullptr;
    unsigned errs = 0;
    int s = 0;
    for (long base = Tpad - 64; base >= 0; base -= 64) {
        const unsigned long long wd = surv[base + lane];
        const int wd_lo = (int)(unsigned)wd, wd_hi = (int)(unsigned)(wd >> 32);
        unsigned long long bits = 0;  // step base + tl at bit 63 - tl: the tile's 8 output bytes, MSB first
#pragma unroll
        for (int tl = 63; tl >= 0; --tl) {
            const unsigned half = (unsigned)__builtin_amdgcn_readlane(tl < 32 ? wd_lo : wd_hi, s);  // state s's lane
            bits |= (unsigned long long)(s >> 5) << (63 - tl);
            s = ((s << 1) & 63) | (int)((half >> (tl & 31)) & 1u);
        }
        // a path into state 0 at step T has six zero inputs before it, and the
        // steps past T stay in state 0: no bit at or past info_bits is ever set
        const long B = (base >> 3) + lane;
        if (lane < 8 && B < nbytes) {
            const unsigned v = (unsigned)(bits >> (56 - 8 * lane)) & 0xffu;
            out[B] = (uint8_t)v;
            if (ref) {
                unsigned rv = ref[B];
                if (rem && B == nbytes - 1) rv &= 0xffu << (8 - rem);
                errs += __popc(v ^ (rv & 0xffu));
            }
        }
    }
    if (a.bit_errors && ref) {
        errs += __shfl_down(errs, 4);
        errs += __shfl_down(errs, 2);
        errs += __shfl_down(errs, 1);
        if (lane == 0 && errs) atomicAdd(a.bit_errors, (unsigned long long)errs);
    }
}

template <class M, bool LDS_SURV>
hipError_t launch_decode(const FecDecArgs& a, hipStream_t stream)
{
    const unsigned grid = (unsigned)((a.ncw + FEC_CW_PER_WG - 1) / FEC_CW_PER_WG);
    const size_t lds = LDS_SURV ? (size_t)FEC_CW_PER_WG * fec_steps_padded(a.info_bits) * 8 : 0;
    if (a.gather == 1)
        hipLaunchKernelGGL((fec_decode_kernel<M, LDS_SURV, 1>), dim3(grid), dim3(DEC_THREADS), lds, stream, a);
    else
        hipLaunchKernelGGL((fec_decode_kernel<M, LDS_SURV, 0>), dim3(grid), dim3(DEC_THREADS), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_fec_encode(const FecEncArgs& a, hipStream_t stream)
{
    const size_t total = (size_t)a.ncw * (size_t)a.coded_stride;
    const size_t grid = (total + ENC_THREADS - 1) / ENC_THREADS;
    if (grid > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fec_encode_kernel, dim3((unsigned)grid), dim3(ENC_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_fec_decode(const FecDecArgs& a, hipStream_t stream)
{
    if ((a.ncw + FEC_CW_PER_WG - 1) / FEC_CW_PER_WG > 0x7fffffffL) return hipErrorInvalidValue;
    const bool lds = a.ws == nullptr;
    if (a.fmt == 1) return lds ? launch_decode<int, true>(a, stream) : launch_decode<int, false>(a, stream);
    return lds ? launch_decode<float, true>(a, stream) : launch_decode<float, false>(a, stream);
}

}  // namespace ofdm
