// ofdm_mac.hip — the batched MAC framing of include/ofdm_mi355x.h ("MAC
// framing and frame check"): header, byte-sum checksum and CRC-32 frame check
// sequence, written and checked one wave per frame. DESIGN.md "MAC framing"
// has the structure, the CRC arithmetic and the measurements; ofdm_mac.hpp the
// per-lane steps, which the host self-test runs too.
#include <hip/hip_runtime.h>
#include "ofdm_mac.hpp"

namespace ofdm {
namespace {

__constant__ MacLanePow mac_lane_pow = mac_make_lane_pow();

__device__ inline unsigned wave_xor(unsigned v)
{
    for (int d = 32; d; d >>= 1) v ^= (unsigned)__shfl_xor((int)v, d);
    return v;
}

__device__ inline unsigned wave_add(unsigned v)
{
    for (int d = 32; d; d >>= 1) v += (unsigned)__shfl_xor((int)v, d);
    return v;
}

// The workgroup's tables: thread v computes entry v of each (no memory is
// read), trow only where a frame has more than one row. The one barrier of a
// launch; the waves then work on their frames without another.
__device__ inline void mac_tabs_init(MacTabs& t, unsigned krow, unsigned rows)
{
    mac_fill_t4(t, threadIdx.x);
    if (rows > 1) mac_fill_trow(t, threadIdx.x, krow);
    __syncthreads();
}

// One wave per frame, several frames after one another. Row by row, every lane
// builds its chunk of the frame (header, payload, zeros), stores it, and adds
// it to its byte sum and its CRC register; the chunks that hold cs or the FCS
// wait. The wave then joins sums and registers, and the lanes that hold those
// chunks build them again with cs and the FCS in place. WIDE: both buffers
// and both strides are 4-byte aligned: a chunk is one 16-byte load and one
// 16-byte store; otherwise a byte.
template <bool WIDE, bool CRC>
__global__ __launch_bounds__(MAC_THREADS) void mac_write_kernel(MacWriteArgs a)
{
    __shared__ MacTabs tabs;
    constexpr unsigned W = WIDE ? 16 : 1;
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned rows = mac_rows(a.frame_len, W);
    const unsigned nchunks = (a.frame_len + W - 1) / W;
    if constexpr (CRC) mac_tabs_init(tabs, a.k.krow, rows);
    const unsigned lpow = mac_lane_pow.p[WIDE ? 1 : 0][lane];
    const unsigned fcs_c0 = a.m / W, fcs_c1 = (a.m + 3) / W;

    for (size_t f = (size_t)blockIdx.x * MAC_WAVES + w; f < a.nframes; f += (size_t)gridDim.x * MAC_WAVES) {
        const uint8_t* pl = a.payload + f * a.payload_stride;
        uint8_t* out = a.frames + f * a.frame_stride;
        const unsigned seq = a.seqs ? (unsigned)a.seqs[f] : (a.seq0 + (unsigned)f) & 0xffffu;
        const unsigned hdr_lo = a.tx_id | (a.rx_id << 16), hdr_hi = seq;
        unsigned sum = 0, crc = 0;
        for (unsigned r = 0; r < rows; ++r) {
            const unsigned c = r * 64 + lane;
            unsigned wd[4] = {0u, 0u, 0u, 0u};
            if (c < nchunks) {
                mac_build_chunk<WIDE>(pl, a.payload_len, hdr_lo, hdr_hi, c, wd);
                const bool waits = c == 6 / W || c == 7 / W || (CRC && c >= fcs_c0 && c <= fcs_c1);
                if (!waits) mac_store_chunk<WIDE>(out, c, wd, a.frame_stride);
                sum += mac_byte_sum(wd[0]) + mac_byte_sum(wd[1]) + mac_byte_sum(wd[2]) + mac_byte_sum(wd[3]);
            }
            if constexpr (CRC) {
                if (r) crc = mac_lookup(tabs.trow, crc);
                crc = mac_crc_chunk<WIDE>(tabs, crc, wd);
            }
        }
        const unsigned cs = wave_add(sum) & 0xffffu;
        if constexpr (CRC) {
            crc = wave_xor(mac_gf_mul(crc, lpow));
            crc = mac_gf_mul(crc, a.k.invz) ^ mac_gf_mul(mac_lookup(tabs.t4, cs << 16), a.k.csadv) ^ a.k.fin;
        }
        // lane i < 2: byte 6 + i; lane 2 + i: FCS byte i. The first lane of a chunk writes it.
        if (lane < (CRC ? 6u : 2u)) {
            const unsigned off = lane < 2 ? 6 + lane : a.m + lane - 2;
            const unsigned c = off / W;
            const unsigned before = lane == 0 ? ~0u : (lane == 2 ? 7u : off - 1) / W;
            if (c != before) {
                unsigned wd[4];
                mac_build_chunk<WIDE>(pl, a.payload_len, hdr_lo, hdr_hi, c, wd);
                mac_place<WIDE>(wd, c, 6, cs, 2);
                if (CRC) mac_place<WIDE>(wd, c, a.m, crc, 4);
                mac_store_chunk<WIDE>(out, c, wd, a.frame_stride);
            }
        }
        // zeros up to the stride
        const unsigned zero[4] = {0u, 0u, 0u, 0u};
        for (size_t c = (size_t)nchunks + lane; c * W < a.frame_stride; c += 64)
            mac_store_chunk<WIDE>(out, c, zero, a.frame_stride);
    }
}

// One wave per frame: one pass loads the frame, sums it, runs the CRC over it
// and copies the payload out; lane 0 then writes the verdict. WIDE: frames,
// payload_out (where given) and both strides are 4-byte aligned: a chunk is
// one 16-byte load and one 16-byte store; otherwise a byte.
template <bool WIDE, bool CRC>
__global__ __launch_bounds__(MAC_THREADS) void mac_read_kernel(MacReadArgs a)
{
    __shared__ MacTabs tabs;
    constexpr unsigned W = WIDE ? 16 : 1;
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned rows = mac_rows(a.frame_len, W);
    if constexpr (CRC) mac_tabs_init(tabs, a.k.krow, rows);
    const unsigned lpow = mac_lane_pow.p[WIDE ? 1 : 0][lane];

    for (size_t f = (size_t)blockIdx.x * MAC_WAVES + w; f < a.nframes; f += (size_t)gridDim.x * MAC_WAVES) {
        const uint8_t* in = a.frames + f * a.frame_stride;
        uint8_t* pl = a.payload ? a.payload + f * a.payload_stride : nullptr;
        MacReadAcc acc{0u, 0u, 0u, 0u, 0u};
        for (unsigned r = 0; r < rows; ++r) {
            if constexpr (CRC)
                if (r) acc.crc = mac_lookup(tabs.trow, acc.crc);
            mac_read_chunk<WIDE, CRC>(tabs, in, pl, a.frame_len, a.m, r * 64 + lane, acc);
        }
        const unsigned cs_calc = wave_add(acc.sum) & 0xffffu;
        const unsigned hdr_lo = wave_xor(acc.hdr_lo), hdr_hi = wave_xor(acc.hdr_hi);
        unsigned fcs_ok = 1;
        if constexpr (CRC) {
            const unsigned fcs = wave_xor(acc.fcs);
            const unsigned crc = mac_gf_mul(wave_xor(mac_gf_mul(acc.crc, lpow)), a.k.invz) ^ a.k.fin;
            fcs_ok = crc == fcs;
        }
        const unsigned cs_ok = (hdr_hi >> 16) == cs_calc;
        const bool ok = cs_ok && fcs_ok && (a.expect_rx_id < 0 || (hdr_lo >> 16) == (unsigned)a.expect_rx_id);
        if (lane == 0) {
            if (a.info) a.info[f] = MacU4{hdr_lo, hdr_hi, cs_calc | (cs_ok << 16) | (fcs_ok << 24), ok ? 1u : 0u};
            if (a.frame_errors && !ok) atomicAdd(a.frame_errors, 1ull);
        }
    }
}

unsigned mac_grid(size_t nframes)
{
    const size_t g = (nframes + MAC_WAVES - 1) / MAC_WAVES;
    return (unsigned)(g < (size_t)MAC_MAX_GRID ? g : (size_t)MAC_MAX_GRID);
}

bool aligned(const void* p, size_t stride, unsigned n) { return !(((uintptr_t)p | (uintptr_t)stride) & (n - 1)); }

}  // namespace

hipError_t launch_mac_write(MacWriteArgs a, bool crc, hipStream_t stream)
{
    const bool wide = aligned(a.frames, a.frame_stride, 4) && aligned(a.payload, a.payload_stride, 4);
    a.k = mac_crc_consts(a.frame_len, a.frame_len - a.m, wide);
    const dim3 grid(mac_grid(a.nframes)), block(MAC_THREADS);
    if (wide) {
        if (crc) hipLaunchKernelGGL((mac_write_kernel<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mac_write_kernel<true, false>), grid, block, 0, stream, a);
    } else {
        if (crc) hipLaunchKernelGGL((mac_write_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mac_write_kernel<false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_mac_read(MacReadArgs a, bool crc, hipStream_t stream)
{
    const bool wide = aligned(a.frames, a.frame_stride, 4) && (!a.payload || aligned(a.payload, a.payload_stride, 4));
    a.k = mac_crc_consts(a.frame_len, a.frame_len - a.m, wide);
    const dim3 grid(mac_grid(a.nframes)), block(MAC_THREADS);
    if (wide) {
        if (crc) hipLaunchKernelGGL((mac_read_kernel<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mac_read_kernel<true, false>), grid, block, 0, stream, a);
    } else {
        if (crc) hipLaunchKernelGGL((mac_read_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mac_read_kernel<false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace ofdm
