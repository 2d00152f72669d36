// ofdm_interleave.hip — the block interleaver (packed bits, int8 and float
// LLRs, both directions) and the additive scrambler of include/ofdm_mi355x.h
// ("interleaver and scrambler"). DESIGN.md "Interleaver and scrambler" has the
// structure, the LDS layout and the measurements.
#include "ofdm_internal.hpp"
#include "ofdm_interleave.hpp"

namespace ofdm {
namespace {

constexpr int IL_THREADS = 256;
constexpr unsigned IL_LDS_MAX = 65536;       // dynamic LDS a launch may ask for without a function attribute
constexpr unsigned IL_TILE_BYTES = 16384;    // small blocks: this many bytes of them per workgroup
constexpr unsigned IL_TILE_BYTES_BITS = 4096;  // (packed bits: 8 gathers per byte)

struct IlDev {
    const unsigned char* in;
    unsigned char* out;
    long nblocks;
    int n, c, rows, s;
    unsigned block_bytes;   // of one block in memory
    unsigned bpw;           // blocks per workgroup
    IlPad pad;
};

// A workgroup stages bpw consecutive blocks (one contiguous run of memory) in
// LDS, padded by a.pad, and every thread then gathers the values of VEC
// consecutive output units from the image: a unit is one element, or one byte
// of 8 packed bits. WIDE: both buffers and every tile start are 16-byte
// aligned, the run is loaded and stored 16 bytes per lane (a tile's last
// bytes, where it is no multiple of 16, element by element); otherwise one
// unit per lane, still coalesced.
template <int KIND, int DIR, bool WIDE>
__global__ __launch_bounds__(IL_THREADS) void il_kernel(IlDev a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char il_lds[];
    constexpr unsigned ES = KIND == IL_F32 ? 4 : 1;    // bytes per unit
    constexpr unsigned PPU = KIND == IL_BITS ? 8 : 1;  // block positions per unit
    constexpr unsigned VEC = WIDE ? 16 / ES : 1;
    const long blk0 = (long)blockIdx.x * a.bpw;
    const long left = a.nblocks - blk0;
    const unsigned nb = left < (long)a.bpw ? (unsigned)left : a.bpw;
    const unsigned tbytes = nb * a.block_bytes;
    const unsigned char* gin = a.in + (size_t)blk0 * a.block_bytes;
    unsigned char* gout = a.out + (size_t)blk0 * a.block_bytes;

    if constexpr (WIDE) {
        for (unsigned o = threadIdx.x * 16; o < tbytes; o += IL_THREADS * 16) {
            if (o + 16 <= tbytes) {
                const uint4 v = *reinterpret_cast<const uint4*>(gin + o);
                *reinterpret_cast<unsigned*>(il_lds + a.pad.at(o)) = v.x;
                *reinterpret_cast<unsigned*>(il_lds + a.pad.at(o + 4)) = v.y;
                *reinterpret_cast<unsigned*>(il_lds + a.pad.at(o + 8)) = v.z;
                *reinterpret_cast<unsigned*>(il_lds + a.pad.at(o + 12)) = v.w;
            } else {
                for (unsigned x = o; x < tbytes; ++x) il_lds[a.pad.at(x)] = gin[x];
            }
        }
    } else {
        for (unsigned o = threadIdx.x * ES; o < tbytes; o += IL_THREADS * ES) {
            if constexpr (ES == 4)
                *reinterpret_cast<unsigned*>(il_lds + a.pad.at(o)) = *reinterpret_cast<const unsigned*>(gin + o);
            else
                il_lds[a.pad.at(o)] = gin[o];
        }
    }
    __syncthreads();

    const unsigned tunits = tbytes / ES;
    for (unsigned u0 = threadIdx.x * VEC; u0 < tunits; u0 += IL_THREADS * VEC) {
        const unsigned pos0 = u0 * PPU;
        unsigned blk = 0, p = pos0;
        if (nb > 1) {
            blk = pos0 / (unsigned)a.n;
            p = pos0 - blk * (unsigned)a.n;
        }
        IlWalk<DIR> w(a.c, a.rows, a.s, (int)p);
        unsigned base = blk * a.block_bytes;  // of the walk's block in the tile
        unsigned wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (unsigned r = 0; r < VEC; ++r) {
            unsigned val = 0;
            if (u0 + r < tunits) {
                if constexpr (KIND == IL_F32) {
                    val = *reinterpret_cast<const unsigned*>(il_lds + a.pad.at(base + 4u * (unsigned)w.src()));
                    if (w.next()) base += a.block_bytes;
                } else if constexpr (KIND == IL_I8) {
                    val = il_lds[a.pad.at(base + (unsigned)w.src())];
                    if (w.next()) base += a.block_bytes;
                } else {
#pragma unroll
                    for (int bit = 0; bit < 8; ++bit) {
                        const unsigned sp = (unsigned)w.src();
                        const unsigned byte = il_lds[a.pad.at(base + (sp >> 3))];
                        val |= ((byte >> (7u - (sp & 7u))) & 1u) << (7 - bit);
                        if (w.next()) base += a.block_bytes;
                    }
                }
            }
            if constexpr (ES == 4) wd[r] = val;
            else wd[r >> 2] |= val << (8u * (r & 3u));
        }
        if (WIDE && u0 + VEC <= tunits) {
            *reinterpret_cast<uint4*>(gout + (size_t)u0 * ES) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        } else {
#pragma unroll
            for (unsigned r = 0; r < VEC; ++r) {
                if (u0 + r < tunits) {
                    if constexpr (ES == 4) *reinterpret_cast<unsigned*>(gout + (size_t)(u0 + r) * 4) = wd[r];
                    else gout[u0 + r] = (unsigned char)(wd[r >> 2] >> (8u * (r & 3u)));
                }
            }
        }
    }
}

// Float blocks whose image does not fit IL_LDS_MAX: one thread per output
// element gathers from memory (the block, 64 to 128 KB, is read once from HBM
// and then served by the L2); stores are coalesced 4-byte.
template <int DIR>
__global__ __launch_bounds__(IL_THREADS) void il_direct_f32_kernel(IlDev a)
{
    const size_t gid = (size_t)blockIdx.x * IL_THREADS + threadIdx.x;
    if (gid >= (size_t)a.nblocks * (size_t)a.n) return;
    const size_t blk = gid / (size_t)a.n;
    const int p = (int)(gid - blk * (size_t)a.n);
    const IlWalk<DIR> w(a.c, a.rows, a.s, p);
    const unsigned* in = reinterpret_cast<const unsigned*>(a.in);
    reinterpret_cast<unsigned*>(a.out)[gid] = in[blk * (size_t)a.n + (size_t)w.src()];
}

// ---------------------------------------------------------------- scrambler
// s_t = s_{t-4} ^ s_{t-7} is an m-sequence of period 127: every seed's
// sequence is the all-ones seed's, started at another phase. seq holds two
// periods of that sequence, MSB first (bit t of the stream at bit 63 - t%64
// of word t/64), so the 8 bits from any phase 0..126 lie in two adjacent
// words; phase[v] is the step at which the register (s_{t-1} .. s_{t-7} at
// bits 0 .. 6) holds v.
struct ScrTab {
    unsigned long long seq[4];
    unsigned char phase[128];
};

constexpr ScrTab make_scr_tab()
{
    ScrTab t{};
    unsigned st = 127;
    for (int i = 0; i < 254; ++i) {
        if (i < 127) t.phase[st] = (unsigned char)i;
        const unsigned b = ((st >> 3) ^ (st >> 6)) & 1u;
        if (b) t.seq[i >> 6] |= 1ull << (63 - (i & 63));
        st = ((st << 1) | b) & 127u;
    }
    return t;
}

__constant__ ScrTab scr_tab = make_scr_tab();

constexpr int SCR_THREADS = 256;

// One thread per output unit: a byte, or (WORD: both buffers and both strides
// 4-byte aligned) a 32-bit word of four, the last bytes of a codeword whose
// length is no multiple of 4 one by one. The unit's sequence bits start at
// phase (phase[seed] + 8*B) mod 127, B its first byte.
template <bool WORD>
__global__ __launch_bounds__(SCR_THREADS) void scramble_kernel(ScrArgs a)
{
    constexpr size_t W = WORD ? 4 : 1;
    const size_t nbytes = (size_t)((a.nbits + 7) >> 3);
    const size_t upc = (nbytes + W - 1) / W;  // units per codeword
    const size_t gid = (size_t)blockIdx.x * SCR_THREADS + threadIdx.x;
    if (gid >= (size_t)a.ncw * upc) return;
    const size_t cw = gid / upc;
    const size_t B = (gid - cw * upc) * W;
    unsigned seed = a.seed;
    if (a.seeds) seed = ((unsigned)a.seeds[cw] + 126u) % 127u + 1u;  // ((v - 1) mod 127) + 1
    const unsigned ph = (scr_tab.phase[seed] + (unsigned)(B % 127u) * 8u) % 127u;
    const unsigned wi = ph >> 6, off = ph & 63u;
    unsigned long long x = scr_tab.seq[wi] << off;  // sequence bits ph .. ph + 63 (< 254), MSB first
    if (off) x |= scr_tab.seq[wi + 1] >> (64u - off);
    const unsigned seq = (unsigned)(x >> 32);
    const unsigned rem = (unsigned)(a.nbits & 7);
    const unsigned last_mask = rem ? (0xffu << (8u - rem)) & 0xffu : 0xffu;
    const unsigned char* in = a.in + cw * (size_t)a.in_stride + B;
    unsigned char* out = a.out + cw * (size_t)a.out_stride + B;
    if (WORD && B + 4 <= nbytes) {
        unsigned v = *reinterpret_cast<const unsigned*>(in) ^ __builtin_bswap32(seq);  // byte B is the low byte
        if (B + 4 == nbytes) v &= (last_mask << 24) | 0x00ffffffu;
        *reinterpret_cast<unsigned*>(out) = v;
    } else {
        const unsigned nb = WORD ? (unsigned)(nbytes - B) : 1u;
        for (unsigned i = 0; i < nb; ++i) {
            unsigned v = ((unsigned)in[i] ^ (seq >> (24u - 8u * i))) & 0xffu;
            if (B + i == nbytes - 1) v &= last_mask;
            out[i] = (unsigned char)v;
        }
    }
}

bool pow2(unsigned x) { return x && !(x & (x - 1)); }
unsigned log2u(unsigned x) { return 31u - (unsigned)__builtin_clz(x); }

// The padding of the staged image: what makes the lanes of one
// gather instruction fall into different banks for c = 16.
IlPad il_pad_for(const IlArgs& a)
{
    const unsigned none = 31;
    if (a.dir == 0) {
        // lane l gathers output units 16 bytes apart: sources 16*c bytes apart
        const unsigned w = 16u * (unsigned)a.c;
        return pow2(w) ? IlPad{log2u(w), 4} : IlPad{none, 0};
    }
    // int8 and bits: the lanes of one instruction read consecutive bytes of one column
    const unsigned rows = (unsigned)(a.n / a.c);
    if (a.kind == IL_F32 && pow2(rows) && rows >= 32) return IlPad{log2u(rows) + 2, 8};
    return IlPad{none, 0};
}

unsigned gcdu(unsigned x, unsigned y) { return y ? gcdu(y, x % y) : x; }

template <int KIND, int DIR>
void il_launch(const IlDev& d, bool wide, unsigned grid, size_t lds, hipStream_t stream)
{
    if (wide) hipLaunchKernelGGL((il_kernel<KIND, DIR, true>), dim3(grid), dim3(IL_THREADS), lds, stream, d);
    else hipLaunchKernelGGL((il_kernel<KIND, DIR, false>), dim3(grid), dim3(IL_THREADS), lds, stream, d);
}

}  // namespace

hipError_t launch_interleave(const IlArgs& a, hipStream_t stream)
{
    IlDev d{};
    d.in = static_cast<const unsigned char*>(a.in);
    d.out = static_cast<unsigned char*>(a.out);
    d.nblocks = a.nblocks;
    d.n = a.n;
    d.c = a.c;
    d.rows = a.n / a.c;
    d.s = a.s;
    d.block_bytes = a.kind == IL_BITS ? (unsigned)a.n / 8 : a.kind == IL_I8 ? (unsigned)a.n : (unsigned)a.n * 4;
    d.pad = il_pad_for(a);
    if (d.pad.at(d.block_bytes) + 16 > IL_LDS_MAX) {
        if (a.kind != IL_F32) return hipErrorInvalidValue;  // (no such block: IL_MAX_BLOCK bytes fit)
        const size_t grid = ((size_t)a.nblocks * (size_t)a.n + IL_THREADS - 1) / IL_THREADS;
        if (grid > 0x7fffffffu) return hipErrorInvalidValue;
        if (a.dir == 0) hipLaunchKernelGGL(il_direct_f32_kernel<0>, dim3((unsigned)grid), dim3(IL_THREADS), 0, stream, d);
        else hipLaunchKernelGGL(il_direct_f32_kernel<1>, dim3((unsigned)grid), dim3(IL_THREADS), 0, stream, d);
        return hipGetLastError();
    }
    long bpw = (long)((a.kind == IL_BITS ? IL_TILE_BYTES_BITS : IL_TILE_BYTES) / d.block_bytes);
    if (bpw < 1) bpw = 1;
    if (bpw > a.nblocks) bpw = a.nblocks;
    const long g = 16 / (long)gcdu(16, d.block_bytes);  // tiles of a multiple of g blocks start 16-byte aligned
    if (bpw >= g) bpw -= bpw % g;
    d.bpw = (unsigned)bpw;
    const long ntiles = (a.nblocks + bpw - 1) / bpw;
    if (ntiles > 0x7fffffffL) return hipErrorInvalidValue;
    const bool wide = !(((uintptr_t)a.in | (uintptr_t)a.out) & 15) && (ntiles == 1 || (bpw * d.block_bytes) % 16 == 0);
    const size_t lds = d.pad.at((unsigned)bpw * d.block_bytes) + 16;
    const unsigned grid = (unsigned)ntiles;
    switch (a.kind * 2 + a.dir) {
    case IL_BITS * 2 + 0: il_launch<IL_BITS, 0>(d, wide, grid, lds, stream); break;
    case IL_BITS * 2 + 1: il_launch<IL_BITS, 1>(d, wide, grid, lds, stream); break;
    case IL_I8 * 2 + 0: il_launch<IL_I8, 0>(d, wide, grid, lds, stream); break;
    case IL_I8 * 2 + 1: il_launch<IL_I8, 1>(d, wide, grid, lds, stream); break;
    case IL_F32 * 2 + 0: il_launch<IL_F32, 0>(d, wide, grid, lds, stream); break;
    case IL_F32 * 2 + 1: il_launch<IL_F32, 1>(d, wide, grid, lds, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_scramble(const ScrArgs& a, hipStream_t stream)
{
    const bool word = !(((uintptr_t)a.in | (uintptr_t)a.out | (uintptr_t)a.in_stride | (uintptr_t)a.out_stride) & 3);
    const size_t nbytes = (size_t)((a.nbits + 7) >> 3);
    const size_t total = (size_t)a.ncw * (word ? (nbytes + 3) / 4 : nbytes);
    const size_t grid = (total + SCR_THREADS - 1) / SCR_THREADS;
    if (grid > 0x7fffffffu) return hipErrorInvalidValue;
    if (word) hipLaunchKernelGGL(scramble_kernel<true>, dim3((unsigned)grid), dim3(SCR_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(scramble_kernel<false>, dim3((unsigned)grid), dim3(SCR_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ofdm
