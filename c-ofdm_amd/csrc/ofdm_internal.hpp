// ofdm_internal.hpp — kernel argument blocks and launcher declarations shared
// by ofdm_kernels.hip (device code) and ofdm_capi.cpp (the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <vector>

namespace ofdm {

// The forward twiddle table W_n^j = exp(-2*pi*i*j/n), j < n, of every FFT
// context (DevTables::tw and the sync kernels' tables; load_twiddles builds
// the two-level LDS table from it). Host code; shared with the test-only
// launchers (devtest/ofdm_devtest.hip), so the table is under test too.
inline std::vector<double2> twiddles(int n)
{
    std::vector<double2> w(n);
    for (int j = 0; j < n; ++j) {
        const double a = 2.0 * M_PI * (double)j / (double)n;
        w[j] = make_double2(std::cos(a), -std::sin(a));
    }
    return w;
}

// Per-context constant tables, resident in HBM (tiny; L2-resident in practice).
struct DevTables {
    const double2* tw;          // N forward twiddles exp(-2*pi*i*j/N)
    const int* data_bin;        // D: FFT bin of data index d within a symbol
    const int* data_slot;       // D: pilot slot j = d / seg owning data index d
    const int* pilot_bin;       // P
    const int* bin_map;         // N: >=0 data index, -1 unused bin, -2 pilot
    const int* rx_pack;         // max(D, RX_DPT*N/8): lds_swz(data_bin) | data_slot << 16, 0-padded
    const int* pilot_swz;       // max(P, N/8): lds_swz(pilot_bin), 0-padded
    const int* tx_code;         // N: tx per-bin code (tx_code_data / tx_code_fixed)
    const double2* constell;    // 2^k mapping table (Modulation::constell)
};

struct TxArgs {
    DevTables tab;
    const uint8_t* bytes;       // nframes * bytes_per_frame
    const double2* points;      // nullable: mapped points instead of bytes (FFT_FORM::write)
    double2* iq;                // frame f message at iq + f*frame_stride (+ msg_offset)
    int16_t* iq16;              // nullable, same indexing, 2 x int16 per sample
    const double2* header;      // T2+preamble samples (nullable: message only)
    long nframes;
    long frame_stride;          // samples
    long msg_offset;            // samples from frame start to the message
    int header_len;             // samples of header to copy per frame
    int S, D, P, cp, k;
    long bytes_per_frame;
    double pilot_ampl;
    double inv_sqrt_n;
    double mult;
    // AWGN (noise_std <= 0: off)
    double noise_scale;         // noise_std / sqrt(2)
    unsigned long long seed;
    unsigned long long sample_offset;
    // one mask per wave of the workgroup (tx_dead_masks); null: every group is mapped
    const unsigned* tx_dead;
};

// The staged stream decode's ramp table, per frame and message symbol:
// CORR_PER_SYM phasors {e^{iA}, e^{iB 2^j} (j < CORR_BITS), e^{iBN/8}}. A
// thread's start phasor e^{i(A + B t)} is e^{iA} times the powers its index
// bits select (t < 2^CORR_BITS = 512 = the largest N/8): products of table
// entries, no sincos in the rx, whose register window leaves no room for one.
constexpr int CORR_BITS = 9;
constexpr int CORR_PER_SYM = CORR_BITS + 2;  // double2 entries

struct RxArgs {
    DevTables tab;
    const double2* iq;          // frame f message at iq + f*frame_stride
    const short2* iq16;         // or: complex<int16> input, same indexing (FRAME_FORM::form_int16_to_double fused)
    long nframes;
    long frame_stride;
    const double2* chan;        // nullable: D divisors per frame
    long chan_stride;           // complex elements between frames (0 = shared)
    bool chan_recip;            // chan holds the divisors' reciprocals (multiply instead of divide)
    double2* constell;          // nullable
    double2* read_out;          // nullable (with chan): FFT_FORM::read's points, before the channel divisor
    uint8_t* bytes;             // nullable
    const uint8_t* ref;         // nullable
    unsigned long long* bit_errors;  // nullable
    double2* ystage;            // staged variant only: nframes*S*D scratch
    // stream mode (staged stream decode): frame f's message body starts at
    // starts[f] + start_off, and message symbol s is multiplied by the phase
    // ramp e^{i(A + B m)} (freq_shift + cp_freq_sinh + pr_phase_sinh) whose
    // table is corr[(f*S + s)*CORR_PER_SYM ..] (ofdm_sync.hip stream_params_kernel)
    const long* starts;         // nullable
    long start_off;
    const long* count;          // nullable: frames beyond min(*count, nframes) are skipped
    int* queue;                 // nullable: {next, done} counters (zero; left zero) for dynamic frames
    const double2* corr;
    int S, D, P, seg, cp, k;
    long bytes_per_frame;
    double pilot_ampl;
    // the emit's fast path (hard decisions of k = 2 as threshold compares,
    // output words assembled in the wave): the context's thresholds of
    // decide_select (ofdm_dev.hpp decide_tau_scan); dec_fast = 0: not offered
    double dec_tau[3];
    int dec_fast;
};

// The soft rx's own arguments (rx_soft_kernel's second parameter: RxArgs and
// with it every rx_kernel instantiation stay as they are).
struct SoftArgs {
    void* llr;                  // nframes*S*D*k LLRs: float (OFDM_LLR_F32) or int8 (OFDM_LLR_I8)
    const double* frame_scale;  // nullable, device: frame f uses scale * frame_scale[f]
    double scale;
    int fmt;
};

// Launchers (ofdm_kernels.hip). Return hipSuccess or the launch error.
hipError_t launch_rx_soft(int logn, const RxArgs& a, const SoftArgs& sa, hipStream_t stream);
hipError_t launch_soft_demap(const double2* pts, long n, int k, double scale, int fmt, void* out, hipStream_t stream);
hipError_t launch_tx(int logn, const TxArgs& a, hipStream_t stream);
hipError_t launch_rx(int logn, const RxArgs& a, hipStream_t stream, bool* staged_needed);
// decide_tau_scan for k in {2, 4}: out = 3 thresholds + the checks' verdict (4 doubles, device)
hipError_t launch_decide_tau_scan(int k, double* out, hipStream_t stream);
hipError_t launch_copy(void* dst, const void* src, size_t n, hipStream_t stream);  // kernel copy (device / mapped pinned)
hipError_t launch_demap(double2* pts, long n, int k, uint8_t* bytes, hipStream_t stream);
hipError_t launch_map(const uint8_t* bytes, long nbytes, int k, const double2* table, double2* out,
                      hipStream_t stream);
hipError_t launch_bit_convert(const uint8_t* in, long len, int in_bits, int out_bits, uint8_t* out, long out_len,
                              hipStream_t stream);
hipError_t launch_i16_to_f64(const int16_t* in, long n, double* out, hipStream_t stream);
hipError_t launch_f64_to_i16(const double* in, long n, double mult, int16_t* out, hipStream_t stream);

// Register-resident rx limits: S*ceil(D/T) <= RX_REG_SLOTS.
constexpr int RX_SMAX = 8;
// LDS slot of FFT element e (ofdm_fft.hpp lds_swz), for host-built tables
inline int lds_swz_host(int e) { return e ^ ((e >> 3) & 7); }
constexpr int RX_DPT = 4;
// rx: persistent resident waves per CU (2 per SIMD: the register window's occupancy)
constexpr int RX_WAVES_PER_CU = 8;
// tx per-bin code: bits 0-12 data index d, bits 13-20 mask applied to its
// k-bit payload symbol (0xff data, 0 otherwise), bits 21-29 base entry of the
// tx kernel's LDS point table (0 for data; TX_LDS_PILOT / TX_LDS_ZERO hold the
// pilot amplitude and 0), so every bin maps as table[(bits(d) & mask) + base].
constexpr int TX_LDS_PILOT = 256, TX_LDS_ZERO = 257;
inline int tx_code_data(int d) { return d | (0xff << 13); }
inline int tx_code_fixed(int entry) { return entry << 21; }
// tx dead groups: thread t of the N/8 holds bins t + (N/8) i, i < 8, so wave w
// holds, as its register group i, the 64 bins 64 w + lane + (N/8) i. Bit i of
// mask w is set when all of them are TX_LDS_ZERO entries (guard band or bin
// 0): the kernel then neither loads nor maps the group, and its first
// butterfly drops the additions of those zeros. No masks for N < 512 (less
// than a wave of threads).
inline std::vector<unsigned> tx_dead_masks(const std::vector<int>& tx_code)
{
    const int T = (int)tx_code.size() / 8;
    std::vector<unsigned> m(T / 64, 0u);
    for (int w = 0; w < T / 64; ++w)
        for (int i = 0; i < 8; ++i) {
            bool dead = true;
            for (int lane = 0; lane < 64; ++lane) dead = dead && tx_code[64 * w + lane + T * i] == tx_code_fixed(TX_LDS_ZERO);
            if (dead) m[w] |= 1u << i;
        }
    return m;
}
// tx: persistent grid-stride launch size (symbols per workgroup = nsym / grid)
constexpr long TX_MAX_GRID = 4096;


// ---- channel code (ofdm_fec.hip): K=7 133/171 encoder, soft-input Viterbi
// Puncturing of the mother stream: keep bit (i % period) of `mask`; `kept`
// of every `period` mother bits are transmitted. The kept positions of a
// period are 0, 1, 2 and (rate 3/4) 5.
struct FecRate { int period, kept; unsigned mask; };
__host__ __device__ inline FecRate fec_rate(int rate)
{
    return rate == 0 ? FecRate{1, 1, 0x1u} : rate == 1 ? FecRate{4, 3, 0x7u} : FecRate{6, 4, 0x27u};
}
constexpr int FEC_TAIL = 6;
constexpr long FEC_MAX_INFO_BITS = 1L << 20;
constexpr int FEC_CW_PER_WG = 4;        // one wave64 per codeword
constexpr long FEC_LDS_STEPS = 1024;    // survivors stay in LDS up to this many (padded) trellis steps
// trellis steps of a codeword, rounded up to the decoder's 64-step tiles (one survivor word each)
inline long fec_steps_padded(long info_bits) { return (info_bits + FEC_TAIL + 63) & ~63L; }

struct FecEncArgs {
    const uint8_t* info;
    uint8_t* coded;
    long info_stride, coded_stride;   // bytes
    long ncw, info_bits, coded_bits;
    int rate;
};

struct FecDecArgs {
    const void* llr;                  // float (OFDM_LLR_F32) or int8 (OFDM_LLR_I8)
    long llr_stride;                  // elements
    long ncw, info_bits;
    unsigned long long* ws;           // survivors, fec_steps_padded words per codeword (LDS where null)
    uint8_t* out;
    const uint8_t* ref;               // nullable
    unsigned long long* bit_errors;   // nullable
    long info_stride;                 // bytes (out and ref)
    int fmt, rate;
    int gather;                       // predecessor gather: 0 ds_bpermute, 1 LDS write + 8-byte pair read
};

hipError_t launch_fec_encode(const FecEncArgs& a, hipStream_t stream);
hipError_t launch_fec_decode(const FecDecArgs& a, hipStream_t stream);


// ---- interleaver and scrambler (ofdm_interleave.hip)
constexpr long IL_MAX_BLOCK = 32768;    // positions of one block
enum { IL_BITS = 0, IL_I8 = 1, IL_F32 = 2 };

struct IlArgs {
    const void* in;
    void* out;
    long nblocks;
    int n, c, s;                      // block positions, columns, rotation group (validated by the caller)
    int kind;                         // IL_BITS (MSB-first packed bits), IL_I8, IL_F32
    int dir;                          // 0 forward, 1 inverse
};

struct ScrArgs {
    const uint8_t* in;
    uint8_t* out;
    const uint8_t* seeds;             // nullable: one seed per codeword
    long in_stride, out_stride;       // bytes
    long ncw, nbits;
    unsigned seed;                    // 1..127, used where seeds is null
};

hipError_t launch_interleave(const IlArgs& a, hipStream_t stream);
hipError_t launch_scramble(const ScrArgs& a, hipStream_t stream);

}  // namespace ofdm
