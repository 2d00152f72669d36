/*
 * ofdm_mi355x.h — C-ABI of the MI355X-native OFDM modem core.
 *
 * This is the drop-in boundary for the reference's DSP layer (DmSM-1/C-OFDM,
 * OFDM/Frame.{hpp,cpp} + OFDM/modulation.{hpp,cpp} + config/parser.{hpp,cpp}).
 * The reference exposes a C++ class surface and no C ABI; each
 * entry point below names the reference member it replaces (file:line,
 * relative to the reference root). The C++ compatibility layer in
 * c-ofdm_amd/compat/ re-exposes that class surface on top of these calls.
 *
 * Conventions
 *   - Every function returns an int status: OFDM_OK (0) or a negative
 *     OFDM_ERR_* code; ofdm_last_error() gives a thread-local message.
 *   - Complex samples are interleaved FP64 {re, im} (the std::complex<double>
 *     layout of the reference and of its data/<name>.bin files).
 *   - Batched compute entry points take DEVICE pointers and an explicit HIP
 *     stream passed as void* (NULL = the legacy default stream). They are
 *     asynchronous.
 *   - Graph capture. The batched compute calls (tx_modulate, tx_frames,
 *     rx_demod and its _i16 / _read / _soft forms, map, demap, soft_demap,
 *     fec_encode, fec_decode, interleave_bits, interleave_llr, scramble, fft_write, fft_read, bit_convert,
 *     int16_to_double, double_to_int16, t2_scan, find_preamble, cfo_estimate,
 *     freq_shift, cp_sync, phase_sync, sync_chain, chan_estimate, sync_frames,
 *     chan_estimate_ls, soft_demap_csi, mac_write, mac_read)
 *     and ofdm_copy only launch kernels on `stream`: no
 *     allocation, no host copy, no synchronisation, and every per-launch
 *     device counter is left as the next launch needs it. A chain of them can
 *     be captured into a hipGraph on one stream and replayed
 *     (tests/test_gpu_graph.py). Three of them allocate context scratch the
 *     first time a context sees a size, so make the same call once before
 *     the capture:
 *       - ofdm_rx_demod* without constell_out on a staged geometry
 *         (num_symb > 8): a scratch of nframes frames, grown when a call asks
 *         for more frames than any call before it;
 *       - ofdm_sync_frames with OFDM_SYNC_CFO and cfo_out = NULL: nframes
 *         doubles, grown likewise;
 *       - ofdm_cfo_estimate / ofdm_sync_frames on a form length (nsym) the
 *         context has not seen: its tables are built and uploaded.
 *     On a stream that is being captured these first calls return
 *     OFDM_ERR_UNSUPPORTED before anything is issued (the capture stays
 *     valid). Not capturable: ofdm_preamble_corr (it stages `start` from the
 *     host and synchronises the stream; OFDM_ERR_UNSUPPORTED on a capturing
 *     stream), ofdm_rx_stream* (the host waits for the walk's status word),
 *     ofdm_reduce_counters, and the memcpy / synchronize / event helpers,
 *     which are plain HIP calls with HIP's own capture rules.
 *   - One ofdm_ctx per thread (or per GPU); a ctx is not re-entrant, matching
 *     the reference (one FRAME_FORM per thread).
 *   - Streams: rx launches keep their frame-queue counter per HIP stream, so
 *     one ctx may run rx / fft_read on several streams at once. The detector
 *     entry points (find_t2sin, find_preamble) and the stream receiver keep
 *     one scratch per ctx: a ctx has at most one of those calls in flight at
 *     a time (consecutive calls on one stream are always fine); overlapping
 *     them on two streams takes two contexts (measured slower than one
 *     context's back-to-back calls: INTEGRATION.md). A stream call waits (on
 *     the device) for the previous stream call's decode when it is issued on
 *     another stream.
 */
#ifndef OFDM_MI355X_H
#define OFDM_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_MI355X_ABI_VERSION 5

enum {
    OFDM_OK = 0,
    OFDM_ERR_INVALID = -1,     /* bad argument / geometry the kernels do not cover */
    OFDM_ERR_UNSUPPORTED = -2, /* valid reference config this build does not run   */
    OFDM_ERR_HIP = -3,         /* HIP runtime error (no GPU, launch failure, ...)  */
    OFDM_ERR_IO = -4,          /* config/file I/O (reference throws runtime_error) */
    OFDM_ERR_NOMEM = -5,
    OFDM_ERR_PARSE = -6        /* std::stol failure in parse_config                */
};

/*
 * Flat view of the ConfigMap keys the hot path consumes
 * (config/parser.hpp:8, consumed in OFDM/Frame.cpp:99-118,157-176,213-232,259-273).
 * Integer-coded fixed point is kept as in config.txt: pilot_ampl/1000,
 * pr_level/1000, t2_sin_level/1000. Missing keys read as 0, as with the
 * reference's ConfigMap::operator[].
 */
typedef struct ofdm_params {
    long fft_size;       /* N */
    long num_data_subc;  /* D */
    long num_pilot_subc; /* P */
    long cp_size;
    long num_symb;       /* message symbols per frame */
    long num_pr_symb;    /* preamble symbols */
    long pr_sin_len;     /* preamble correlation template length */
    long pr_seed;        /* std::mt19937 seed of the preamble bytes */
    long pr_level;       /* /1000: preamble detection threshold */
    long t2sin_size;     /* T2 marker length = detector block */
    long t2_sin_f1;
    long t2_sin_f2;
    long t2_sin_level;   /* /1000: T2 energy-ratio threshold */
    long smooth;         /* T2 mask half-width */
    long mod_type;       /* bits per symbol: 1 bpsk, 2 qam4, 4 qam16, 6 qam64, 8 qam256 */
    long pilot_ampl;     /* /1000: transmitted pilot amplitude */
    long mult;           /* int16 wire scaling (FRAME_FORM::get_int16) */
    long rx_buf_size;    /* rx ring = frame * (rx_buf_size + 1) */
    long iterations;     /* rx.cpp loop count (not used by the core) */
} ofdm_params;

/* Derived frame geometry (FRAME_FORM ctor, OFDM/Frame.cpp:213-232). */
typedef struct ofdm_geometry {
    long symbol_len;       /* N + cp (OFDM_FORM::ofdm_len)                       */
    long message_len;      /* (N+cp)*num_symb  (message.size)                   */
    long preamble_len;     /* (N+cp)*num_pr_symb (preamble.size)                */
    long frame_len;        /* T2 + preamble + message (FRAME_FORM::output_size) */
    long ring_len;         /* frame_len*(rx_buf_size+1) (from_sdr_buf.size())   */
    long data_per_frame;   /* D*num_symb constellation points (message.usefull_size) */
    long bytes_per_frame;  /* D*num_symb*k/8 (FRAME_FORM::usefull_size)         */
    long segment_size;     /* D/P data carriers between pilots                  */
    long pilot_bin[256];   /* pilot FFT bins of one symbol (first P entries)    */
    long segment_bin[256]; /* first FFT bin of each data segment                */
} ofdm_geometry;

/* Optional AWGN channel fused into the tx kernel (bench/loopback only; the
 * reference's channel is the radio, python_code/channel.py). Counter-based
 * noise: identical sample index -> identical noise on every GPU/rank. */
typedef struct ofdm_channel {
    double noise_std;        /* std of the complex noise per time sample (total power) */
    unsigned long long seed;
    unsigned long long sample_offset; /* global index of this batch's first sample */
} ofdm_channel;

typedef struct ofdm_ctx ofdm_ctx;

/* ---- errors / version -------------------------------------------------- */
const char* ofdm_last_error(void);
int ofdm_abi_version(void);

/* ---- config (config/parser.cpp:4-33, config/config.txt) ---------------- */
/* The committed config/config.txt values. */
int ofdm_params_default(ofdm_params* out);
/* parse_config(path) + the config["..."] lookups of the Frame ctors.
 * Returns OFDM_ERR_IO if the file cannot be opened ("Cannot open config
 * file"), OFDM_ERR_PARSE where std::stol would throw. Unknown keys ignored. */
int ofdm_params_from_config(const char* path, ofdm_params* out);
/* Read one raw key the way ConfigMap::operator[] would (0 when missing). */
int ofdm_config_lookup(const char* path, const char* key, long* value);

/* ---- context ----------------------------------------------------------- */
/* Builds every constant the FRAME_FORM ctor builds (Frame.cpp:213-232):
 * pilot/segment tables (Frame.cpp:31-44), T2 marker (Frame.cpp:139-154),
 * preamble bytes/symbol/template (Frame.cpp:259-294), T2 mask (Frame.cpp:120-133),
 * FFT twiddle tables; uploads them to `device`. */
int ofdm_create(const ofdm_params* params, int device, ofdm_ctx** out);
int ofdm_destroy(ofdm_ctx* ctx);
int ofdm_get_geometry(const ofdm_ctx* ctx, ofdm_geometry* out);
/* 1 if this context's batched rx takes the threshold-compare emit (QPSK; the
 * decision thresholds were found and verified on the device at creation)
 * wherever a launch's arguments allow it, 0 if it keeps the decision
 * arithmetic, negative for a null context. */
int ofdm_rx_emit_fast(const ofdm_ctx* ctx);
/* tx's dead groups: a wave of the tx kernel whose 64 bins of one register
 * group all lie in the guard band skips that group's mapping, and its first
 * butterfly drops the additions of those zeros (same samples; fft_size >= 512).
 * enable = 0 makes this context's tx map every group as before, 1 switches
 * the skipping back on (the default), negative leaves the switch alone.
 * masks_out (nullable, fft_size/512 words) receives the per-wave masks (bit i:
 * bins 64 w + lane + (fft_size/8) i are all unused), codes_out (nullable,
 * fft_size ints) the per-bin codes they were built from (bits 21..29 = 257
 * for an unused bin). Returns 1 if tx skips dead groups now (switched on and
 * some mask non-zero), 0 if not, negative for a null context. */
int ofdm_tx_sparse(ofdm_ctx* ctx, int enable, unsigned* masks_out, int* codes_out);
/* Host copies of the constant frame parts (for FRAME_FORM::buf, get(), preamble.*). */
int ofdm_get_t2_symbol(const ofdm_ctx* ctx, double* out /* t2sin_size complex */);
int ofdm_get_preamble(const ofdm_ctx* ctx,
                      uint8_t* bytes_out /* D*num_pr_symb/8, nullable */,
                      double* ofdm_preamble_out /* preamble_len complex, nullable */,
                      double* mod_preamble_out /* D*num_pr_symb complex, nullable */,
                      double* template_out /* pr_sin_len complex, nullable */);

/* ---- device memory helpers (so hosts need not link HIP) ----------------- */
int ofdm_device_alloc(ofdm_ctx* ctx, size_t bytes, void** dptr);
int ofdm_device_free(ofdm_ctx* ctx, void* dptr);
int ofdm_memcpy_h2d(ofdm_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
int ofdm_memcpy_d2h(ofdm_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
int ofdm_memset_device(ofdm_ctx* ctx, void* dst, int value, size_t bytes, void* stream);
int ofdm_stream_synchronize(ofdm_ctx* ctx, void* stream);
/* Page-locked host memory (DMA-able: copies from / to it are asynchronous). */
int ofdm_host_alloc(ofdm_ctx* ctx, size_t bytes, void** hptr);
int ofdm_host_free(ofdm_ctx* ctx, void* hptr);
/* A non-blocking HIP stream on the ctx's device, and its destruction. */
int ofdm_stream_create(ofdm_ctx* ctx, void** stream);
int ofdm_stream_destroy(ofdm_ctx* ctx, void* stream);
/* Device-to-device copy on a stream; HIP events (timing disabled) to wait
 * for part of a stream's work. */
int ofdm_memcpy_d2d(ofdm_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
/* Copy by a kernel on the stream (no DMA engine): dst and src each device
 * memory or page-locked host memory from ofdm_host_alloc. For the small
 * transfers between a stream's kernels, where a DMA hand-off costs more than
 * the copy. */
int ofdm_copy(ofdm_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
int ofdm_event_create(ofdm_ctx* ctx, void** event);
int ofdm_event_record(ofdm_ctx* ctx, void* event, void* stream);
int ofdm_event_synchronize(ofdm_ctx* ctx, void* event);
int ofdm_event_destroy(ofdm_ctx* ctx, void* event);

/* ---- tx: FRAME_FORM::write (Frame.cpp:235-237) -> OFDM_FORM::write
 *      (Frame.cpp:185-198) -> Modulation::mod (modulation.cpp:39-50) +
 *      FFT_FORM::write (Frame.cpp:54-70), batched over frames ------------- */
/* bytes: nframes * bytes_per_frame (device). iq_out: device, frame f's
 * message starts at iq_out + 2*f*frame_stride (complex samples; stride >=
 * message_len). Each symbol is [CP | body], body = IFFT(pilots+data)/sqrt(N).
 * iq16_out (nullable, device): the same samples as complex<int16>
 * trunc(x*mult) — FRAME_FORM::get_int16 (Frame.cpp:249-256), same stride.
 * ch (nullable, host struct): AWGN added to iq_out only. */
int ofdm_tx_modulate(ofdm_ctx* ctx, const uint8_t* bytes, size_t nframes,
                     double* iq_out, size_t frame_stride, int16_t* iq16_out,
                     const ofdm_channel* ch, void* stream);

/* Full FRAME_FORM buffers: [T2 | preamble | message] per frame (output_size
 * samples, contiguous frames), i.e. what FRAME_FORM::get() returns. */
int ofdm_tx_frames(ofdm_ctx* ctx, const uint8_t* bytes, size_t nframes,
                   double* frames_out, int16_t* frames16_out, void* stream);

/* ---- rx: OFDM_FORM::fft (Frame.hpp:276-282) -> FFT_FORM::read
 *      (Frame.cpp:73-96) [-> caller's constell /= chan (main.cpp:69-71)]
 *      -> Modulation::demod (modulation.cpp:53-87), batched over frames ---- */
/* iq: device, frame f's message (num_symb [CP|body] symbols) at
 * iq + 2*f*frame_stride. chan (nullable, device): per-frame D complex
 * divisors (chan_stride complex between frames; 0 = one shared vector).
 * constell_out (nullable): nframes*D*num_symb complex, equalised points
 * BEFORE demod's clamp (data/constell.bin layout). bytes_out (nullable):
 * nframes*bytes_per_frame. ref_bytes + bit_errors (both nullable, device):
 * accumulate popcount(bytes ^ ref_bytes) into *bit_errors (u64 atomic). */
int ofdm_rx_demod(ofdm_ctx* ctx, const double* iq, size_t nframes, size_t frame_stride,
                  const double* chan, size_t chan_stride,
                  double* constell_out, uint8_t* bytes_out,
                  const uint8_t* ref_bytes, unsigned long long* bit_errors,
                  void* stream);

/* ofdm_rx_demod on wire-format input: iq16 = complex<int16> samples (4-byte
 * aligned, device), same frame indexing (FRAME_FORM::from_sdr_int16_buf). The
 * int16 -> double conversion of FRAME_FORM::form_int16_to_double
 * (Frame.hpp:472-481) is exact and fused into the load, so results equal
 * ofdm_rx_demod on the converted samples bit for bit, at 4 B/sample input. */
int ofdm_rx_demod_i16(ofdm_ctx* ctx, const int16_t* iq16, size_t nframes, size_t frame_stride,
                      const double* chan, size_t chan_stride,
                      double* constell_out, uint8_t* bytes_out,
                      const uint8_t* ref_bytes, unsigned long long* bit_errors,
                      void* stream);

/* ofdm_rx_demod with a channel divisor that also writes FFT_FORM::read's
 * points before the division (read_out, npts per frame): one launch for
 * rx.cpp:211-220 (message.fft(), the host loop dividing by chan_char_lq(),
 * Modulation::demod). read_out and constell_out may be page-locked host
 * memory from ofdm_host_alloc (the kernel writes it directly). */
int ofdm_rx_demod_read(ofdm_ctx* ctx, const double* iq, size_t nframes, size_t frame_stride,
                       const double* chan, size_t chan_stride,
                       double* read_out, double* constell_out, uint8_t* bytes_out,
                       void* stream);

/* Modulation::demod alone on n points (modulation.cpp:53-87): clamps `points`
 * IN PLACE for QAM (as the reference does) and writes n*k/8 bytes (rounded up,
 * last byte left-aligned as bit_stream_converter pads). Device pointers. */
int ofdm_demap(ofdm_ctx* ctx, double* points, size_t n, uint8_t* bytes_out, void* stream);
/* ---- soft decisions: max-log LLRs of the reference's own constellation
 * (modulation.cpp:4-36: natural binary per axis, not Gray), computed in FP64
 * from the equalised point z BEFORE demod's clamp (the point constell_out
 * holds: after the pilot gains and after the caller-side channel division).
 * For bit b of z's k-bit symbol, MSB first (bit_stream_converter's order):
 *
 *   L_b = s * ( min_{c: bit_b(c)=1} |z-c|^2 - min_{c: bit_b(c)=0} |z-c|^2 )
 *
 * L_b > 0 means bit 0; s is the caller's scale (e.g. 1/N0). QAM is separable:
 * the symbol is col | row*m, m = 2^(k/2); bits 0..k/2-1 come from the
 * imaginary axis (row), bits k/2..k-1 from the real axis (col), both with PAM
 * levels l_j = 2j/(m-1) - 1. BPSK (k = 1): L_0 = -2*sqrt(2)*(re + im)*s (its
 * points (+-1+-j)/sqrt(2) lie on the diagonal, modulation.cpp:28-30).
 * k = 1, 2, 4, 6, 8; any other k: OFDM_ERR_UNSUPPORTED.
 * Output llr[point*k + b], points in constell_out order, so LLR i of a frame
 * belongs to bit i of that frame's bytes_out stream:
 *   OFDM_LLR_F32: (float)L_b, round to nearest (llr_out 4-byte aligned);
 *   OFDM_LLR_I8 : (int8) clamp(rint(L_b), -127, 127), rint half-to-even on
 *                 the FP64 value.
 * Stores are widest where llr_out is 16-byte aligned. OFDM_ERR_INVALID: null
 * llr_out, unknown fmt, scale not finite or <= 0, misaligned buffers.
 * Not covered: the stream decodes (run ofdm_soft_demap on their constell_out)
 * and the compat layer (the reference has no soft surface). */
enum { OFDM_LLR_F32 = 0, OFDM_LLR_I8 = 1 };

/* n points -> n*k LLRs. points (device, 16-byte aligned) is NOT modified
 * (unlike ofdm_demap). */
int ofdm_soft_demap(ofdm_ctx* ctx, const double* points, size_t n, double scale,
                    int fmt, void* llr_out, void* stream);

/* ofdm_rx_demod / ofdm_rx_demod_i16 (exactly one of iq, iq16) that also
 * writes the LLRs of every equalised point: nframes*D*num_symb*k elements.
 * Frame f uses s = scale * frame_scale[f] (frame_scale: nullable, device,
 * nframes doubles, read by the kernel: a captured graph follows a changing
 * SNR), or scale alone. constell_out, bytes_out, ref_bytes and bit_errors are
 * ofdm_rx_demod's, with bit-identical values. Every geometry ofdm_rx_demod
 * accepts; asynchronous; capturable (a staged geometry without constell_out
 * after one call outside the capture, as ofdm_rx_demod). */
int ofdm_rx_demod_soft(ofdm_ctx* ctx, const double* iq, const int16_t* iq16,
                       size_t nframes, size_t frame_stride,
                       const double* chan, size_t chan_stride,
                       double scale, const double* frame_scale,
                       int fmt, void* llr_out,
                       double* constell_out, uint8_t* bytes_out,
                       const uint8_t* ref_bytes, unsigned long long* bit_errors,
                       void* stream);

/* ---- frequency-selective channels: a per-carrier least-squares channel
 * estimate from the preamble, and LLRs weighted by the channel state. The
 * receive chain (INTEGRATION.md "Frequency-selective channels"):
 *     ofdm_sync_frames, ofdm_chan_estimate_ls on the synced preamble,
 *     ofdm_rx_demod(chan = H, constell_out), ofdm_soft_demap_csi,
 *     ofdm_interleave_llr, ofdm_fec_decode, ofdm_scramble.
 *
 * ofdm_chan_estimate_ls. x, nframes and frame_stride are ofdm_chan_estimate's
 * (below): frame f's preamble form, num_pr_symb [CP|body] symbols, starts at
 * x + 2*f*frame_stride and is not modified. With D = num_data_subc:
 *   input points   pr[s*D + c] = FFT_FORM::read of the preamble form
 *                  (Frame.cpp:73-96 on its num_pr_symb symbols: phys over the
 *                  form's own pilots, the per-segment coef against symbol 0),
 *                  the points ofdm_chan_estimate starts from;
 *   preamble points m = mod_preamble (ofdm_get_preamble), D per symbol;
 *   raw estimate   raw[c] = (1/num_pr_symb) * sum_s pr[s*D+c] / m[s*D+c],
 *                  s ascending;
 *   smoothing      half-width w = smooth, 0 <= w <= 64: H[c] = the mean of
 *                  raw[a..b], summed in ascending order and divided by the
 *                  count, a = max(lo, c-w), b = min(hi-1, c+w), where
 *                  [lo, hi) is the half of the data carriers that holds c,
 *                  [0, D/2) or [D/2, D): the two sides of DC in the carrier
 *                  order, the split chan_char_lq makes. w = 0: H = raw.
 *   outputs        chan_out[f*chan_stride + c] = H[c] (complex: a drop-in for
 *                  the `chan` of ofdm_rx_demod*), csi_out[f*csi_stride + c] =
 *                  re(H)^2 + im(H)^2 (one double). Either may be NULL, not
 *                  both; strides in elements, >= D for each output given.
 * The kernel applies 1/phys and 1/num_pr_symb after the sum (phys is known
 * after the last symbol): equal to the definition within 1e-9 * max|H|.
 * Every geometry ofdm_chan_estimate accepts, num_data_subc > fft_size/2
 * included. Asynchronous: no allocation, no host copy, no synchronisation;
 * capturable. OFDM_ERR_INVALID: null x, both outputs null, smooth out of
 * range, a stride below D, misaligned buffers (complex 16, csi_out 8 bytes).
 * OFDM_ERR_UNSUPPORTED, before anything is launched: a geometry whose LDS
 * need (fft_size + fft_size/64 + 80 + num_pr_symb*num_pilot_subc + D complex
 * values) exceeds 160 KB. nframes == 0: OFDM_OK, no launch.
 *
 * ofdm_soft_demap_csi. points: nframes * D * num_symb equalised points in
 * constell_out order (device, 16-byte aligned, not modified); point i of
 * frame f sits on carrier c = i mod D. csi: D doubles per frame at
 * csi + f*csi_stride (csi_stride = 0: one vector shared by every frame).
 * frame_scale: nullable, as ofdm_rx_demod_soft's.
 *   llr[(f*D*num_symb + i)*k + b] = s * (d1 - d0),
 *   s = scale * frame_scale[f] * csi[f*csi_stride + c],
 * d0, d1 the max-log minima of "soft decisions" above. Formats, rounding,
 * saturation and alignment rules are ofdm_soft_demap's.
 * Erasures: a point with a non-finite component, or a weight csi[..] that is
 * not finite and > 0 (zero, negative, inf, NaN), gives exactly 0 for all k
 * LLRs of the point (+0.0 in OFDM_LLR_F32): an H[c] = 0 division in the rx
 * does not send NaN into the decoder.
 * OFDM_ERR_INVALID: null points, csi or llr_out, unknown fmt, scale not
 * finite or <= 0, misaligned buffers, 0 < csi_stride < D.
 * OFDM_ERR_UNSUPPORTED: k outside 1, 2, 4, 6, 8. nframes == 0: OFDM_OK.
 * Asynchronous; capturable.
 * The Viterbi decoder is invariant to a common scale of a codeword's LLRs:
 * only the relative weights of the carriers matter.
 * Not covered: the weight fused into ofdm_rx_demod_soft (the rx kernels are
 * untouched), the stream decodes and the compat layer, a noise-variance
 * estimate, MMSE equalisation, interpolation from the pilots alone. */
int ofdm_chan_estimate_ls(ofdm_ctx* ctx, const double* x, size_t nframes, size_t frame_stride,
                          int smooth, double* chan_out, size_t chan_stride,
                          double* csi_out, size_t csi_stride, void* stream);
int ofdm_soft_demap_csi(ofdm_ctx* ctx, const double* points, size_t nframes,
                        const double* csi, size_t csi_stride,
                        double scale, const double* frame_scale,
                        int fmt, void* llr_out, void* stream);

/* ---- channel code: the rate-1/2, constraint-length-7 convolutional code
 * (generators 133/171 octal, 802.11 / DVB) with its 2/3 and 3/4 puncturings,
 * and a soft-input Viterbi decoder fed by the LLRs above. Definition:
 *
 * Bits are MSB-first within bytes (bit_stream_converter's order). A codeword
 * carries info_bits information bits u_0 .. u_{info_bits-1} followed by 6
 * zero tail bits: T = info_bits + 6 trellis steps. The encoder state is the
 * previous six inputs, the most recent at bit 5. At step t:
 *     reg = (u_t << 6) | state
 *     A_t = parity(reg & 0133),  B_t = parity(reg & 0171)
 *     state = reg >> 1
 * The mother stream is m[2t] = A_t, m[2t+1] = B_t (a single 1 followed by
 * zeros gives A = 1011011, B = 1111001, weight 10). Puncturing keeps mother
 * index i in [0, 2T) where keep[i mod period] is 1:
 *     OFDM_FEC_R12  period 1  {1}
 *     OFDM_FEC_R23  period 4  {1,1,1,0}
 *     OFDM_FEC_R34  period 6  {1,1,1,0,0,1}
 * coded_bits(info_bits, rate) is the number of kept indices; transmitted bit
 * n of a codeword is the n-th kept mother bit.
 *
 * The decoder takes one LLR per transmitted bit (L > 0 means bit 0;
 * OFDM_LLR_F32 or OFDM_LLR_I8), counts punctured positions as L = 0, and
 * gives the information bits of the trellis path with the largest metric
 * sum (1 - 2 c_n) L_n among the paths that start in state 0 and end in state
 * 0 after T steps. Tie rule: new state s' has the predecessors
 * p_j = ((2 s') & 63) | j, j = 0, 1; when both candidates are equal, j = 0
 * survives; a candidate from a state not reachable from state 0 always loses
 * to a reachable one. With int8 input the metrics are integers and the output
 * is exactly defined. The decisions do not change under a positive scale of
 * a codeword's LLRs: the soft calls' scale only sets the int8 quantisation,
 * and frame_scale matters only to decoders that are not scale-invariant.
 * Not covered: tail-biting, other codes, the stream
 * decodes (run the decoder on LLRs from ofdm_soft_demap of their
 * constell_out) and the compat layer (the reference has no channel code). */
enum { OFDM_FEC_R12 = 0, OFDM_FEC_R23 = 1, OFDM_FEC_R34 = 2 };

/* Host arithmetic (no context, no GPU). coded_bits of one codeword, and the
 * largest info_bits whose coded_bits <= capacity_bits (one codeword per frame:
 * capacity_bits = bytes_per_frame*8); OFDM_ERR_INVALID: null result, unknown
 * rate, info_bits == 0, or no codeword fits. */
int ofdm_fec_coded_bits(size_t info_bits, int rate, size_t* coded_bits);
int ofdm_fec_max_info_bits(size_t capacity_bits, int rate, size_t* info_bits);

/* ncw codewords, device pointers, strides in bytes (info_stride >=
 * ceil(info_bits/8), coded_stride >= ceil(coded_bits/8)). Codeword c is read
 * at info + c*info_stride (bits past info_bits in the last byte are ignored)
 * and exactly coded_stride bytes are written at coded + c*coded_stride: the
 * coded bits MSB-first, then zero bits, so coded_stride = bytes_per_frame
 * feeds ofdm_tx_modulate directly. Asynchronous; capturable. */
int ofdm_fec_encode(ofdm_ctx* ctx, const uint8_t* info, size_t info_stride, size_t ncw,
                    size_t info_bits, int rate, uint8_t* coded, size_t coded_stride,
                    void* stream);

/* Bytes of survivor storage the decoder wants from the caller for ncw
 * codewords of info_bits (0 where the survivors stay in LDS). */
int ofdm_fec_workspace_size(size_t ncw, size_t info_bits, size_t* bytes);

/* Codeword c's LLRs are llr[c*llr_stride ..] (llr_stride in elements, >=
 * coded_bits; elements past coded_bits are not read; F32: 4-byte aligned).
 * Writes ceil(info_bits/8) bytes at info_out + c*info_stride, the last one
 * left-aligned and zero-padded, and nothing else. ref_info (same layout as
 * info_out) and bit_errors (device u64, accumulated atomically as in
 * ofdm_rx_demod) are nullable: the popcount over the info_bits bits only.
 * workspace: device memory, 16-byte aligned, at least the size
 * ofdm_fec_workspace_size gives; may be NULL only where that is 0. No
 * allocation, no host copy, no synchronisation; capturable.
 * OFDM_ERR_INVALID (both batched calls): null required pointers, unknown rate
 * or fmt, info_bits == 0 or > 2^20, strides too small, a missing, misaligned
 * or too-small workspace, a misaligned F32 input. ncw == 0: OFDM_OK, no
 * launch. */
int ofdm_fec_decode(ofdm_ctx* ctx, const void* llr, int fmt, size_t llr_stride, size_t ncw,
                    size_t info_bits, int rate, void* workspace, size_t workspace_bytes,
                    uint8_t* info_out, size_t info_stride, const uint8_t* ref_info,
                    unsigned long long* bit_errors, void* stream);

/* ---- interleaver and scrambler: the two stages between the channel code
 * and the modem. The device-side chain is
 *     tx: ofdm_mac_write, ofdm_scramble, ofdm_fec_encode,
 *         ofdm_interleave_bits (forward), ofdm_tx_modulate
 *     rx: ofdm_rx_demod_soft, ofdm_interleave_llr (inverse), ofdm_fec_decode,
 *         ofdm_scramble, ofdm_mac_read
 * (INTEGRATION.md has the arguments). Every call below that takes a stream is
 * batched, takes device pointers and only launches kernels: no allocation,
 * no host copy, no synchronisation; capturable.
 *
 * The permutation. A block has n = block_bits positions, c = cols columns
 * and a rotation group s. Block position q (0 <= q < n) moves to
 *     i = (n/c) * (q mod c) + floor(q / c)
 *     j = s * floor(i/s) + (i + n - floor(c*i / n)) mod s
 * OFDM_IL_FORWARD writes out[j(q)] = in[q], OFDM_IL_INVERSE out[q] = in[j(q)].
 * The inverse map in closed form:
 *     i = s*floor(j/s) + (j + floor(c*j/n)) mod s
 *     q = c*i - (n-1)*floor(c*i/n)
 * Valid: c >= 1, c | n, s >= 1, s | (n/c), n % 8 == 0, 8 <= n <= 32768. With
 * c = 16 and s = max(k/2, 1) this is the 802.11a interleaver: (48, 16, 1)
 * starts 0, 3, 6, 9, ..., (192, 16, 2) starts 0, 13, 24, 37, 48, 61, ....
 * A frame's blocks are its OFDM symbols, n = num_data_subc * modType; the pad
 * bits behind a frame's codeword are interleaved with everything else.
 *
 * The scrambler is additive, x^7 + x^4 + 1: s_t = s_{t-4} ^ s_{t-7}, with
 * s_{-m} = bit m-1 of the seed for m = 1..7; out bit t = in bit t ^ s_t (bits
 * MSB-first). Seed 127 gives the 802.11 sequence 00001110 11110010 11001001
 * 00000010 ..., period 127. The operation is its own inverse.
 *
 * OFDM_ERR_INVALID (the batched calls): null required pointers, invalid
 * (n, c, s), unknown dir or fmt, strides too small, nbits == 0, a scalar seed
 * outside 1..127, misaligned F32, in and out overlapping (ofdm_scramble: in ==
 * out with other than equal strides). nblocks == 0 or ncw == 0: OFDM_OK, no
 * launch. A grid that does not fit: OFDM_ERR_HIP, nothing launched.
 * Not covered: the deinterleave fused into the decoder or the soft rx (the
 * frame check is ofdm_mac_read, below), the per-carrier weight of ofdm_soft_demap_csi fused into ofdm_rx_demod_soft,
 * a noise-variance estimate, MMSE equalisation, and the compat layer. */
enum { OFDM_IL_FORWARD = 0, OFDM_IL_INVERSE = 1 };

/* Host arithmetic: the context's per-symbol block, num_data_subc*modType
 * positions in 16 columns with s = max(modType/2, 1). OFDM_ERR_UNSUPPORTED
 * where those are no valid parameters. */
int ofdm_interleave_default(const ofdm_ctx* ctx, size_t* block_bits, size_t* cols, size_t* s);

/* nblocks blocks of MSB-first bits, nblocks*block_bits/8 bytes each side. in
 * and out must not overlap; in is not modified. Forward on ofdm_fec_encode's
 * output (coded_stride = bytes_per_frame, nblocks = nframes*num_symb) feeds
 * ofdm_tx_modulate; inverse on the hard rx's bytes_out gives the
 * hard-decision path. */
int ofdm_interleave_bits(ofdm_ctx* ctx, const uint8_t* in, size_t nblocks, size_t block_bits,
                         size_t cols, size_t s, int dir, uint8_t* out, void* stream);

/* The same permutation on elements (fmt: OFDM_LLR_F32, 4-byte aligned, or
 * OFDM_LLR_I8, any address), moved bit for bit: NaN payloads and -0.0 come
 * through unchanged. Loads and stores are widest where both buffers are
 * 16-byte aligned. Inverse on ofdm_rx_demod_soft's llr_out with
 * nblocks = nframes*num_symb gives the layout ofdm_fec_decode takes with
 * llr_stride = bytes_per_frame*8. */
int ofdm_interleave_llr(ofdm_ctx* ctx, const void* in, int fmt, size_t nblocks, size_t block_bits,
                        size_t cols, size_t s, int dir, void* out, void* stream);

/* ncw codewords of nbits, strides in bytes (>= ceil(nbits/8)). Writes exactly
 * ceil(nbits/8) bytes per codeword; the bits past nbits in the last one are
 * written 0. seed in 1..127; seeds (nullable, device, ncw bytes) gives one
 * seed per codeword instead, a value v outside 1..127 counting as
 * ((v-1) mod 127) + 1. in == out with equal strides is allowed. */
int ofdm_scramble(ofdm_ctx* ctx, const uint8_t* in, size_t in_stride, size_t ncw, size_t nbits,
                  unsigned seed, const uint8_t* seeds, uint8_t* out, size_t out_stride, void* stream);

/* ---- MAC framing and frame check: the reference's outermost layer,
 * mac.write(...) before FRAME_FORM::write (main.cpp:37, tx.cpp:34) and
 * mac.read(...) after Modulation::demod (main.cpp:82, rx.cpp:221), batched on
 * the device, with the frame check sequence a coded link needs. A MAC frame is
 * frame_len bytes, F = 4 with OFDM_FCS_CRC32 and 0 with OFDM_FCS_NONE:
 *     0 .. 7                        tx_id, rx_id, seq_num, cs: four uint16,
 *                                   little-endian (the reference's MAC header)
 *     8 .. frame_len-F-1            payload, cap = frame_len - 8 - F bytes; a
 *                                   shorter input is zero-filled (MAC::write)
 *     frame_len-F .. frame_len-1    FCS (OFDM_FCS_CRC32 only)
 * cs is the sum of bytes [0, frame_len-F) without bytes 6 and 7, mod 2^16
 * (MAC::calc_cs; 0x577E on the golden frame). With OFDM_FCS_NONE the frame is
 * bit for bit MAC(tx, rx, frame_len).write(payload, seq). The FCS is
 * CRC-32/IEEE 802.3 (reflected polynomial 0xEDB88320, initial value and final
 * XOR 0xFFFFFFFF: zlib's crc32) of bytes [0, frame_len-4) with cs in place,
 * stored little-endian as the 802.11 FCS is: the CRC-32 of a whole good frame
 * is the residue 0x2144DF1C. Valid: 8 + F <= frame_len <= 65536,
 * payload_len <= cap.
 *
 * The two batched calls take device pointers and only launch one kernel: no
 * allocation, no host copy, no synchronisation; capturable. One wave works on
 * a frame, 16 bytes per lane where both buffers and both strides are 4-byte
 * aligned (fastest 16-byte aligned), a byte per lane otherwise.
 *
 * OFDM_ERR_INVALID: null required pointers, unknown fcs, sizes outside the
 * rules above, strides below the length they carry, ids above 65535, input
 * and output overlapping, a misaligned info_out (16 bytes), frame_errors (8)
 * or seqs (2). These are checked before the context is, and before any device
 * call. nframes == 0: OFDM_OK, no launch. The grid is bounded (the waves
 * stride over the frames), so no launch is too large for it.
 * Not covered: other polynomials, a CRC fused into the decoder or the
 * descrambler, fragmentation, ARQ, addressing beyond the rx_id filter, and the
 * compat layer's MAC class, which stays the host class it is. */
enum { OFDM_FCS_NONE = 0, OFDM_FCS_CRC32 = 1 };

/* ofdm_mac_read's verdict on one frame: 16 bytes, the array 16-byte aligned. */
typedef struct ofdm_mac_info {
    uint16_t tx_id, rx_id, seq_num, cs;   /* as received */
    uint16_t cs_calc;                     /* recomputed */
    uint8_t  cs_ok, fcs_ok;               /* fcs_ok = 1 with OFDM_FCS_NONE */
    uint8_t  ok;                          /* cs_ok && fcs_ok && the rx_id filter */
    uint8_t  reserved[3];                 /* written 0 */
} ofdm_mac_info;

/* Host arithmetic: *cap = frame_len - 8 - F. OFDM_ERR_INVALID for an unknown
 * fcs or a frame_len outside [8 + F, 65536]. */
int ofdm_mac_payload_len(size_t frame_len, int fcs, size_t* cap);

/* nframes frames from payload_len payload bytes each (payload may be NULL
 * where payload_len is 0). Frame f carries seq_num = (seq0 + f) mod 2^16, as
 * tx.cpp counts, or seqs[f] where seqs (nullable, device, nframes uint16) is
 * given. Writes exactly frame_stride bytes per frame, the MAC frame and then
 * zeros (ofdm_fec_encode's coded_stride convention): frame_stride =
 * bytes_per_frame feeds ofdm_tx_modulate, frame_stride = ceil(info_bits/8)
 * feeds ofdm_scramble / ofdm_fec_encode. payload and frames_out must not
 * overlap. */
int ofdm_mac_write(ofdm_ctx* ctx, const uint8_t* payload, size_t payload_stride, size_t payload_len,
                   size_t nframes, size_t frame_len, int fcs, unsigned tx_id, unsigned rx_id,
                   unsigned seq0, const uint16_t* seqs, uint8_t* frames_out, size_t frame_stride,
                   void* stream);

/* Checks nframes received frames in one pass: payload_out (nullable) receives
 * cap bytes per frame, bad frames included, as MAC::read does; info_out
 * (nullable) the header as received and the verdict; *frame_errors (nullable,
 * device, 8-byte aligned) is increased atomically by the number of frames with
 * ok == 0 and is not written where there is none. ok also requires
 * rx_id == expect_rx_id where expect_rx_id >= 0. At least one of the three
 * outputs must be given. The input is not modified and must not overlap an
 * output. */
int ofdm_mac_read(ofdm_ctx* ctx, const uint8_t* frames, size_t frame_stride, size_t nframes,
                  size_t frame_len, int fcs, int expect_rx_id, uint8_t* payload_out,
                  size_t payload_stride, ofdm_mac_info* info_out, unsigned long long* frame_errors,
                  void* stream);

/* Modulation::mod alone (modulation.cpp:39-50): nbytes -> nbytes*8/k points. */
int ofdm_map(ofdm_ctx* ctx, const uint8_t* bytes, size_t nbytes, double* points_out, void* stream);

/* FFT_FORM::write (Frame.cpp:54-70) on given points: per frame, D*num_symb
 * constellation points -> FFT_buf layout (num_symb bodies of N samples, no
 * CP): zero, pilots, segments, unnormalised IFFT, /sqrt(N). Device buffers. */
int ofdm_fft_write(ofdm_ctx* ctx, const double* points, size_t nframes, double* fft_buf, void* stream);
/* FFT_FORM::read (Frame.cpp:73-96) on an FFT_buf layout (num_symb bodies of
 * N samples per frame, no CP) -> restored D*num_symb points per frame. The
 * input is not modified (the reference transforms FFT_buf in place). */
int ofdm_fft_read(ofdm_ctx* ctx, const double* fft_buf, size_t nframes, double* restored, void* stream);

/* Modulation::bit_stream_converter (modulation.cpp:90-125): MSB-first repack
 * of len in_bits-wide units into ceil(len*in_bits/out_bits) out_bits-wide
 * units, last one left-aligned; *out_len receives the count. 1 <= bits <= 8. */
int ofdm_bit_convert(ofdm_ctx* ctx, const uint8_t* in, size_t len, int in_bits, int out_bits,
                     uint8_t* out, size_t* out_len, void* stream);

/* FRAME_FORM::form_int16_to_double (Frame.hpp:472-481): n complex<int16>
 * samples -> n complex<double>. Device buffers. */
int ofdm_int16_to_double(ofdm_ctx* ctx, const int16_t* in, size_t n, double* out, void* stream);

/* FRAME_FORM::get_int16 (Frame.cpp:249-256) on n given samples:
 * complex<int16>(x * complex(mult)) = per-component trunc(x*mult). Device buffers. */
int ofdm_double_to_int16(ofdm_ctx* ctx, const double* in, size_t n, int16_t* out, void* stream);

/* ---- rx sync front end ----------------------------- */
/* T2SIN_FORM::corr (Frame.hpp:96-147) over all floor((n-start)/t2sin_size)
 * blocks from `start`: rel_out[b] = energy ratio if > level else 0 (device,
 * nullable). first_out (device int, or page-locked host int from
 * ofdm_host_alloc; nullable): T2SIN_FORM::find_t2sin (Frame.hpp:150-197) =
 * start + b*size of the first block above level, or -1, written once by the
 * launch's last workgroup (system-scope fence after it: a host thread may
 * poll a pinned first_out instead of synchronising the stream). */
int ofdm_t2_scan(ofdm_ctx* ctx, const double* iq, size_t n, long start,
                 double* rel_out, int* first_out, void* stream);

/* PREAMBLE_FORM::find_preamble (Frame.cpp:338-378) for a batch of starts:
 * idx_out[i] = starts[i] + first lag whose normalised correlation with the
 * preamble template exceeds pr_level/1000 (lags 0 .. 2*T2sin_size+pr_sin_len-1,
 * running window energy updated after each test, as the reference), or -10.
 * Samples past n read as 0, and so do the samples before 0 that a negative
 * start reaches. Device arrays. Callers add +1 (main.cpp:53).
 * nstarts == 0: OFDM_OK, nothing written. Before anything is issued:
 * OFDM_ERR_INVALID for nstarts > 65535 (one launch's limit; split the batch),
 * OFDM_ERR_UNSUPPORTED for a T2sin_size / pr_sin_len pair whose
 * 2*T2sin_size + pr_sin_len lags do not fit one workgroup's 160 KB of LDS
 * (every T2sin_size = 4096, which ofdm_t2_scan accepts; T2sin_size = 2048
 * fits up to pr_sin_len = 664). idx_out is then left as it was. */
int ofdm_find_preamble(ofdm_ctx* ctx, const double* iq, size_t n,
                       const int* starts, size_t nstarts, int* idx_out, void* stream);

/* PREAMBLE_FORM::find_corr (Frame.cpp:297-335): the normalised correlation
 * at every lag from `start` (cor_out[i] = |sum x[start+i+j] c_j| / sqrt(norm_i)
 * where norm_i > 1, else 0; 2*T2sin_size + pr_sin_len lags). Device arrays.
 * Samples past n read as 0, and so do the samples before 0 that a negative
 * start reaches. Unlike the other compute calls this one copies
 * `start` from the host and synchronises `stream` before it returns: it cannot
 * be captured (OFDM_ERR_UNSUPPORTED on a capturing stream).
 * OFDM_ERR_UNSUPPORTED, before the host copy and with cor_out left as it was,
 * for the T2sin_size / pr_sin_len pairs ofdm_find_preamble refuses. */
int ofdm_preamble_corr(ofdm_ctx* ctx, const double* iq, size_t n, long start, double* cor_out,
                       void* stream);

/* ---- per-frame synchronisation, batched over located frames ------------
 * `x` points at the first sample of a form in frame 0; frame f's form starts
 * at x + 2*f*frame_stride. A "form" is nsym consecutive [CP|body] symbols
 * (OFDM_FORM: preamble form nsym = num_pr_symb, message_with_preamble form
 * nsym = num_pr_symb + num_symb). All pointers are device pointers. */

/* OFDM_FORM::pilot_freq_sinh (Frame.hpp:285-337): coarse CFO (cycles/sample)
 * of each frame's form from the pilot peaks of its (N+cp)*nsym-point FFT.
 * Needs (N+cp)*nsym = 2^a or 5*2^a. cfo_out may be pinned host memory
 * (ofdm_host_alloc): each value is written with a system-scope fence, so a
 * caller can poll it instead of synchronising the stream (as ofdm_t2_scan's
 * first_out). */
int ofdm_cfo_estimate(ofdm_ctx* ctx, const double* x, size_t nframes, size_t frame_stride,
                      int nsym, double* cfo_out, void* stream);

/* OFDM_FORM::freq_shift (Frame.hpp:340-348): x[n] *= exp(-2*pi*i*cfo[f]*n),
 * n = 0 .. nsamples-1, in place. cfo: device array of nframes values. */
int ofdm_freq_shift(ofdm_ctx* ctx, double* x, size_t nframes, size_t frame_stride,
                    size_t nsamples, const double* cfo, void* stream);

/* OFDM_FORM::cp_freq_sinh (Frame.hpp:238-263): per-symbol CP-correlation fine
 * CFO, phase-continuous across the nsym symbols of the form, in place. */
int ofdm_cp_sync(ofdm_ctx* ctx, double* x, size_t nframes, size_t frame_stride, int nsym,
                 void* stream);

/* OFDM_FORM::pr_phase_sinh (Frame.hpp:265-274): common phase vs pr[0..pr_len)
 * (device), applied to nsamples samples in place. pr = NULL uses the
 * context's own ofdm_preamble (preamble_len samples), as main.cpp:63 does. */
int ofdm_phase_sync(ofdm_ctx* ctx, double* x, size_t nframes, size_t frame_stride,
                    size_t nsamples, const double* pr, size_t pr_len, void* stream);

/* main.cpp:61-63 after the CFO estimate in one launch: ofdm_freq_shift(cfo),
 * ofdm_cp_sync(nsym), ofdm_phase_sync(pr = NULL), in place on nsamples
 * samples per frame (nsym*(N+cp) <= nsamples; a form up to 158 KB is held in
 * LDS between the stages). x equals the three calls bit for bit; shift_out,
 * cp_out, phase_out (each nullable; device or page-locked host memory from
 * ofdm_host_alloc, frame f at + 2*f*out_stride) receive the form after each
 * stage: the states OFDM_FORM's output[0] holds between the members. */
int ofdm_sync_chain(ofdm_ctx* ctx, double* x, size_t nframes, size_t frame_stride, size_t nsamples,
                    int nsym, const double* cfo, double* shift_out, double* cp_out, double* phase_out,
                    size_t out_stride, void* stream);

/* PREAMBLE_FORM::chan_char_lq (Frame.hpp:389-434): linear-phase channel
 * estimate from the preamble form at x -> chan_out[f*D .. f*D+D) unit phasors
 * (data/phases.bin layout). chan_stride: complex elements between frames. */
int ofdm_chan_estimate(ofdm_ctx* ctx, const double* x, size_t nframes, size_t frame_stride,
                       double* chan_out, size_t chan_stride, void* stream);

/* The main.cpp:60-66 chain on each frame's message_with_preamble region
 * (preamble + message, in place): cfo -> freq_shift -> cp_sync -> phase_sync
 * (context preamble) -> chan_estimate. Clear OFDM_SYNC_* bits to skip a stage
 * (cfo_in, nullable, then supplies the CFO; OFDM_SYNC_FREQ_SHIFT with neither
 * OFDM_SYNC_CFO nor cfo_in: OFDM_ERR_INVALID, nothing launched). Outputs
 * nullable: without cfo_out the estimate goes to a context scratch (allocated
 * by the first call of a given nframes: see "Graph capture" above); without
 * chan_out OFDM_SYNC_CHAN does nothing. Each stage equals its stand-alone call
 * bit for bit. */
enum {
    OFDM_SYNC_CFO = 1, OFDM_SYNC_FREQ_SHIFT = 2, OFDM_SYNC_CP = 4,
    OFDM_SYNC_PHASE = 8, OFDM_SYNC_CHAN = 16, OFDM_SYNC_ALL = 31
};
int ofdm_sync_frames(ofdm_ctx* ctx, double* frames, size_t nframes, size_t frame_stride,
                     int stages, const double* cfo_in, double* cfo_out, double* chan_out,
                     void* stream);

/* ---- streaming rx (rx.cpp:94-221) --------------------------------------
 * Every frame rx.cpp's receive loop locates in a stream of n complex samples
 * (device), then the main.cpp:60-80 chain and demod on each. The walk
 * (rx.cpp:126-198) is, per step:
 *   hit = find_t2sin(pos) (blocks pos + k*T2sin_size); pb = find_preamble(hit) + 1;
 *   pb < -2 -> pos = hit + message_len; else the frame
 *   [pb, pb + preamble_len + message_len) is decoded and pos = pb + message_len.
 * rx.cpp runs it over its SDR ring (from_sdr_buf, rx.cpp:73-91,137-189): the
 * buffer holds output_size + R samples, R = rx_buf_size * output_size (one SDR
 * refill, sdr.hpp:141); find_t2sin only tests blocks that end inside the
 * buffer; a T2 miss refills WITHOUT carrying the tail and restarts the grid
 * at the new buffer, and a hit (preamble) in the buffer's last output_size
 * (+ T2sin_size) samples carries them to the front before the refill. So a
 * marker straddling a refill can be lost, and the grid's phase depends on
 * the ring. The stream API reproduces this exactly (ring mode, the default
 * when the config's rx_buf_size > 0: R from the config; ofdm_set_stream_ring
 * changes R, 0 = no ring, the continuous walk over the stream held whole).
 * In ring mode sample 0 of `iq` is the SDR's first sample and the walk starts
 * as rx.cpp does, at the zero header before it (ofdm_stream_initial_state);
 * samples past n read as zero (the walk ends once its scan passes n).
 * A frame the walk locates past the stream end stops the walk. A frame whose
 * preamble starts before sample 0 (a capture that begins inside it; rx.cpp
 * locates it in its ring's zero header, rx.cpp:105-114,158) is decoded as
 * rx.cpp decodes it, with the samples before 0 read as zero; its pb_out
 * entry is negative.
 * The walk runs as parallel chunk walkers joined into the one sequential
 * walk on the device (chunk = samples per walker, 0 = automatic; see
 * ofdm_walk_tuning). Outputs (device, nullable):
 * pb_out[f] preamble start, bytes_out (bytes_per_frame per frame),
 * constell_out (D*num_symb complex per frame), cfo_out. *nframes_out = frames
 * found; outputs hold the first max_frames. The input is not modified.
 * OFDM_ERR_UNSUPPORTED, before anything is issued (*nframes_out = 0, no output
 * written), for a detector the walker does not take: T2sin_size = 2^a, 64..2048
 * only, and a T2sin_size / pr_sin_len pair whose walker needs more than one
 * workgroup's 160 KB of LDS. The direct preamble search (pr_sin_len > 449)
 * holds 2*T2sin_size + pr_sin_len lags and about 72 bytes per template sample
 * there, so T2sin_size = 2048 is taken up to pr_sin_len = 449 (it has no
 * direct search), 1024 up to 1328 and 512 up to 1785. This is narrower than
 * ofdm_find_preamble's own limit (T2sin_size = 2048 up to pr_sin_len = 664).
 * Returns once the walk is resolved (the host waits for a small status block);
 * the decode is enqueued on `stream` and may still be running, so order later
 * work on `stream`, or synchronise it, before reading the outputs. */
int ofdm_rx_stream(ofdm_ctx* ctx, const double* iq, size_t n, size_t max_frames, long chunk,
                   long* pb_out, uint8_t* bytes_out, double* constell_out, double* cfo_out,
                   size_t* nframes_out, void* stream);
/* ofdm_rx_stream on the SDR's wire format (rx.cpp's from_sdr_int16_buf):
 * iq16 = n complex<int16> samples (device, 4-byte aligned), converted exactly
 * on load; results equal ofdm_rx_stream on the converted stream. */
int ofdm_rx_stream_i16(ofdm_ctx* ctx, const int16_t* iq16, size_t n, size_t max_frames, long chunk,
                       long* pb_out, uint8_t* bytes_out, double* constell_out, double* cfo_out,
                       size_t* nframes_out, void* stream);

/* rx.cpp's SDR ring for the stream walk: R samples per refill (>=
 * output_size), 0 = the continuous walk. Default: rx_buf_size * output_size. */
int ofdm_set_stream_ring(ofdm_ctx* ctx, long ring);
int ofdm_get_stream_ring(const ofdm_ctx* ctx, long* ring);

/* Measurement (no reference counterpart): with on = 1, every later stream
 * call records HIP events around its walk, its resolve and its decode on the
 * call's stream, and ofdm_get_stream_timing returns the last call's three
 * device times in ms (waiting for its decode). The events sit between
 * dependent kernels and cost launch gaps, so time the calls themselves with
 * timing off. Fails when the last call had no timed decode (timing off, the
 * halo walk, or a decode that is not the speculative one). */
int ofdm_set_stream_timing(ofdm_ctx* ctx, int on);
int ofdm_get_stream_timing(ofdm_ctx* ctx, float* walk_ms, float* resolve_ms, float* decode_ms);

/* A state of the stream walk: the position of the next T2 search and, in
 * ring mode, one past the last sample of the ring buffer's current SDR
 * refill (stream coordinates; 0 without a ring). */
typedef struct ofdm_walk_state {
    long pos;
    long ring_end;
} ofdm_walk_state;
/* rx.cpp's initial state (rx.cpp:105-114): ring mode {-output_size, R} (pos 0
 * of a buffer whose zero header precedes the first SDR buffer), else {0, 0}. */
int ofdm_stream_initial_state(const ofdm_ctx* ctx, ofdm_walk_state* out);

/* One shard of a longer stream (multi-GPU streaming rx; the
 * reference's rx.cpp:145-156 carries one frame from ring to ring, this is the
 * same hand-over between GPUs). Exactly one of iq (complex f64) / iq16
 * (complex<int16>) is set; it holds the shard's n samples: its core plus a
 * walk-in halo before it and a tail after it. The walk starts at state
 * `start` (shard-relative; the whole stream's initial state, or the
 * predecessor shard's exit state, or any other state for a speculative walk
 * that the caller checks, see c-ofdm_amd/python/ofdm_stream.py; ring mode
 * also fixes the ring ends' phase: start->ring_end + k*R) and the frames
 * located with pb in [own_lo, own_hi) are decoded into the outputs exactly as
 * ofdm_rx_stream does (pb_out relative to iq). Requires 0 <= own_lo <= own_hi
 * <= n and start->pos >= 0 (ring mode: >= -output_size, start->pos - 2048 -
 * T2sin_size < start->ring_end <= start->pos + R + output_size).
 *   *exit_out: the walk's first state at or past own_hi (where the next
 *     shard's walk resumes; a state equivalent to it, or the state whose step
 *     located the first frame past own_hi), pos -1 if the samples ran out.
 *     In ring mode its pos may lie up to one T2 scan step past its ring end
 *     (a scan that crossed own_hi where the ring runs out: its next step is
 *     the refill); it is a valid start state for the next call.
 *   located (host, nullable, located_cap entries) / located_lag (host,
 *     nullable: ring mode's state after the frame has the later of its two
 *     possible ring ends) / *nlocated_out (nullable): the frames the walk
 *     located from `start` until it stopped: those before own_lo, the owned
 *     ones, and any located past own_hi; *nlocated_out counts them all, and
 *     when they are more than located_cap the arrays hold the first
 *     located_cap - located_cap/2 and the last located_cap/2 of them (what a
 *     shard-to-shard check reads: the walk-in and the frames past own_hi).
 *     Two walks that located the same frame with the same lag are in the
 *     same state from there on. located_cap = 0: no list is made.
 * ofdm_rx_stream(iq, n) is ofdm_rx_stream_shard(iq, n, initial state, 0, n). */
int ofdm_rx_stream_shard(ofdm_ctx* ctx, const double* iq, const int16_t* iq16, size_t n,
                         const ofdm_walk_state* start, long own_lo, long own_hi, size_t max_frames, long chunk,
                         long* pb_out, uint8_t* bytes_out, double* constell_out, double* cfo_out,
                         size_t* nframes_out, long* located, uint8_t* located_lag, size_t located_cap,
                         size_t* nlocated_out, ofdm_walk_state* exit_out, void* stream);

/* Samples a shard of ofdm_rx_stream_shard needs around its core
 * [own_lo, own_hi): *halo_out before own_lo for the walk-in to meet the true
 * walk without a re-walk (the walkers' chunk halo), *tail_out past own_hi for
 * the step that crosses own_hi (one scan step, a T2 block, the preamble
 * window, then the frame). Either pointer may be NULL. */
int ofdm_stream_shard_margins(const ofdm_ctx* ctx, long* halo_out, long* tail_out);

/* ---- multi-GPU (BASELINE configs[4]) -------------------------
 * One process (or thread) per GPU, one ofdm_ctx per GPU. Frames are
 * independent, so a batch shards as contiguous frame ranges with no data-path
 * collective; the job's one collective is a SUM all-reduce of its counters
 * (bit errors, bits, samples, frames) over RCCL (xGMI). A stream shards by
 * samples: each rank walks its core plus a walk-in halo and a tail, and the
 * ranks check their walks against each other with one small exchange
 * (c-ofdm_amd/python/ofdm_stream.py; ofdm_rx_stream_shard). See
 * INTEGRATION.md for the 8-GPU C++ binding (apps/ofdm_multigpu.cpp). */
/* Contiguous share of `total` units for `rank` of `world`, the remainder to
 * the low ranks: [*first, *first + *count). */
int ofdm_shard_range(size_t total, int world, int rank, size_t* first, size_t* count);
/* A stream of n samples sharded by samples: `rank`'s core [*own_lo, *own_hi)
 * and the slice [*slice_lo, *slice_hi) it must hold (the core plus a 3-frame
 * walk-in halo, at least ofdm_stream_shard_margins' halo, and the tail a walk
 * crossing own_hi reads), clipped to [0, n). The plan of ofdm_stream.py's
 * shard_stream. Pure arithmetic on the config: no GPU needed. */
int ofdm_stream_shard_plan(const ofdm_params* params, size_t n, int world, int rank, long* slice_lo,
                           long* slice_hi, long* own_lo, long* own_hi);
/* The job's one collective: SUM all-reduce, in place, of `count` int64
 * counters in device memory over an RCCL communicator (ncclComm_t passed as
 * void*; every rank calls it), enqueued on `stream`. RCCL (librccl.so) is
 * loaded at the first call; without it OFDM_ERR_UNSUPPORTED. */
int ofdm_reduce_counters(ofdm_ctx* ctx, int64_t* counters, size_t count, void* nccl_comm, void* stream);
/* Visible HIP devices (0 and OFDM_ERR_HIP without a GPU). */
int ofdm_device_count(int* count);

/* The sharded stream's report exchange (the protocol of
 * c-ofdm_amd/python/ofdm_stream.py, which these restate for C/C++ hosts).
 * Each rank walks its slice (ofdm_rx_stream_shard: rank 0 from the stream's
 * initial state, the others speculatively from their slice start with the
 * first ring end after it), packs a fixed-size report row, and the ranks
 * all-gather the rows (one ncclAllGather of int64). Every rank then runs the
 * same plan on the same rows: the first rank whose walk is not yet known to
 * be the true walk re-walks from the state the plan returns (its
 * predecessor's exit state), re-packs its row with true_start = 1, and the
 * exchange repeats until the plan accepts every rank. The union of the owned
 * frames is then exactly the one sequential walk's (rx.cpp:125-221).
 * Row length in int64: OFDM_STREAM_REPORT_HEADER + 2 * cap. */
#define OFDM_STREAM_REPORT_HEADER 7
/* Pack a report row. located / located_lag: the walk's located frames in
 * walk order (ABSOLUTE preamble starts: ofdm_rx_stream_shard's relative ones
 * plus slice_lo) and their ring lags (NULL: all 0), nlocated of them, as
 * ofdm_rx_stream_shard returns them with located_cap = 2 * cap (the walk's
 * first and last cap frames when longer); exit_state absolute (pos -1: the
 * samples ran out); true_start: the walk started from a state of the true
 * walk (rank 0, or a re-walk). row: OFDM_STREAM_REPORT_HEADER + 2 * cap. */
int ofdm_stream_report_pack(int rank, long slice_lo, long own_lo, long own_hi, const long* located,
                            const uint8_t* located_lag, size_t nlocated, const ofdm_walk_state* exit_state,
                            int true_start, size_t cap, int64_t* row);
/* The plan over the world's rows (rank order, each packed with the same
 * cap): *rank_out = the first rank to re-walk and *start_out the absolute
 * state to re-walk it from (pos -1: the true walk ended before that rank's
 * core, so it and the ranks after it own no frame), or *rank_out = -1 when
 * every walk is accepted. Rank r is accepted when it was walked from a true
 * state, or when it and rank r-1 located a common frame (same preamble start
 * and lag) no later than r's first owned frame. t2sin_size: the config's
 * (an exit state before the slice moves forward on its own T2 grid). */
int ofdm_stream_stitch_plan(const int64_t* rows, int world, size_t cap, long t2sin_size, int* rank_out,
                            ofdm_walk_state* start_out);

/* ---- stream walk tuning (tests and experiments) --------------------------
 * Per-context settings of the ofdm_rx_stream* walkers; ofdm_create sets the
 * defaults (ofdm_walk_tuning_default), which are the product configuration.
 * chunks_per_slot, halo_milli, ext_milli and lookback change only how the
 * walk is split over walkers: the stitched walk is exact for any values.
 * lookback = 1 (default): each chunk's walker starts at its core (minus
 * halo_milli, default 0) and walks on past the core end until its walk
 * shares a frame with the records the next chunk's walker has published;
 * the chain of joined walks, resolved on the device, is the sequential walk
 * (no host stitching, no re-walks). lookback = 0: every chunk walks in from a
 * halo (default 3 frames) and the host stitches the walks, re-walking a chunk
 * whose walk-in missed the true walk (short halos cost serial re-walks).
 * halo_milli = -1 selects the mode's default. exact_search = 1 replaces the certified FFT
 * preamble search by the reference's serial recurrence; t2_f32 = 0 turns the
 * FP32 T2 screen off (FP64 only). t2_margin is the FP32 screen's
 * certification margin: at or above the default 4e-5 every uncertain block is
 * decided in FP64. A smaller margin would trust raw FP32 ratios near the
 * level and could make the walk differ from the reference, so it is refused
 * (OFDM_ERR_INVALID) unless allow_uncertified = 1, a test-only switch (the
 * tests compare margin 0 against the certified screen). staged_decode = 1
 * decodes through the three staged kernels instead of the one fused decode
 * kernel (same results within the parity bar; for A/B measurements). */
typedef struct ofdm_walk_tuning {
    long chunks_per_slot; /* chunks per resident walker (>= 1; default 1)       */
    long halo_milli;      /* walk-in halo, 1/1000 frames (-1 = default: 0 with
                             lookback, 3000 without)                            */
    long ext_milli;       /* walk-on past the core end, 1/1000 frames (0)       */
    int exact_search;     /* 1: serial-recurrence preamble search (default 0)   */
    int t2_f32;           /* 1: certified FP32 T2 screen (default 1)            */
    double t2_margin;     /* FP32 screen margin (default 4e-5, the certified minimum) */
    int allow_uncertified; /* test only: 1 accepts t2_margin < 4e-5 (default 0) */
    int staged_decode;    /* 1: decode located frames with the staged cfo ->
                             params -> rx kernels even where a fused decode
                             kernel fits (A/B measurements, tests; default 0) */
    int lookback;         /* 1: device-side look-back stitching (default 1)     */
    int max_rec_cap;      /* test only: > 0 caps the records per walker (forces
                             the look-back overflow and its halo-walk fallback;
                             default 0 = the computed bound)                    */
    int pre_f32;          /* 1: certified FP32 tier of the FFT preamble search
                             (an uncertain lag is re-decided in FP64; default 1) */
} ofdm_walk_tuning;
int ofdm_walk_tuning_default(ofdm_walk_tuning* out);
int ofdm_get_walk_tuning(const ofdm_ctx* ctx, ofdm_walk_tuning* out);
int ofdm_set_walk_tuning(ofdm_ctx* ctx, const ofdm_walk_tuning* tuning);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_H */
